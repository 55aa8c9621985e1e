"""On-device ensemble products (C ABI ``msw_ensemble_steps_update``, ``msw_ensemble_maps``):
a rollout reduced across the members of an ensemble.

The flood maps (``mswegnn.floodmaps``) reduce a rollout over time, the zone series
(``mswegnn.series``) over space; this module reduces over members.  An ensemble is one mesh run
with M boundary hydrographs, breach locations or initial states -- a batch of M copies of one graph
(:func:`make_ensemble`), at most ``MAX_ENSEMBLE_MEMBERS`` = 64 -- and what is delivered from it is
probabilistic maps: the probability that the depth exceeds a threshold, the p10 / p50 / p90 of the
peak depth, the step by which half of the members are wet.  Two HIP kernels do it where the rollout
lives: a streaming one for per-step statistics across members (:class:`EnsembleSteps`) and a
one-shot one for order statistics across members of per-member maps (:func:`ensemble_maps`,
:class:`EnsembleMaps`).  :func:`rollout_ensemble` feeds both from a chunked rollout that is never
held whole.  The reference has no counterpart.

Member order is the order of the row ranges given; every sum and every tie-break follows it.
Quantiles are numpy's ``inverted_cdf`` ones (:func:`quantile_rank`): a member's own value, never
an interpolation.

Scores (C ABI ``msw_ensemble_scores_update``): :class:`EnsembleScores` verifies the ensemble
against a truth run where both live -- the CRPS, the reliability table and the Brier score at the
thresholds, the spread against the error of the ensemble mean -- from sums whose order of addition
depends on the cell count alone, so that a rollout scored in chunks gives the bits of the whole.
The scores are those of the M-member empirical distribution: E|X - y| - E|X - X'| / 2 with both
expectations over the members (the "fair" CRPS would divide the second by M (M - 1) instead of
M^2), and the spread is the population one (the unbiased variance is M / (M - 1) times its square).

On CPU tensors the same interface runs :func:`_steps_torch` / :func:`_maps_torch` /
:func:`_scores_torch`, plain torch restatements.
"""
from __future__ import annotations

import ctypes as C
import math
from fractions import Fraction

import torch

from . import _lib as L
from .batch import collate
from .floodmaps import FloodMaps, _over_60, rollout_chunks
from .metrics import finest_ranges
from .rollout import adapt_batch_training

__all__ = ["STEP_NAMES", "SCORE_NAMES", "quantile_rank", "make_ensemble", "member_ranges", "EnsembleSteps",
           "ensemble_maps", "EnsembleMaps", "EnsembleScores", "ensemble_scores", "rollout_ensemble"]

STEP_NAMES = ("wet_members", "h_mean", "h_min", "h_max")
SCORE_NAMES = ("sums", "reliability", "cell_crps")
SCORE_SUMS = ("a", "b", "abs_e", "e2", "v")
_VALUE_MAPS = ("h_max", "q_max", "vel_max", "froude_max")
_INT_MAX = torch.iinfo(torch.int32).max


def quantile_rank(p, M):
    """The rank (0 = smallest of ``M``) of the ``p``-quantile: ``ceil(p M) - 1`` clipped to
    0..M-1, numpy's ``inverted_cdf``.  ``p`` is taken as the exact decimal it prints as
    (``Fraction(str(p))``): the float product can round up past an integer -- 0.07 * 100 is
    7.000000000000001 in float64 -- and shift the rank."""
    M = int(M)
    if M < 1:
        raise ValueError("M must be at least 1")
    q = Fraction(str(p))
    if not 0 <= q <= 1:
        raise ValueError(f"probability {p} outside [0, 1]")
    return min(max(math.ceil(q * M) - 1, 0), M - 1)


def make_ensemble(graph, bcs, xs=None):
    """M clones of ``graph`` as one batch, already passed through ``adapt_batch_training``: member
    m takes ``BC = bcs[m]`` (the shape of ``graph.BC``) and, with ``xs``, ``x = xs[m]``."""
    M = len(bcs)
    if not 1 <= M <= L.MAX_ENSEMBLE_MEMBERS:
        raise ValueError(f"an ensemble has 1..{L.MAX_ENSEMBLE_MEMBERS} members, not {M}")
    if xs is not None and len(xs) != M:
        raise ValueError("xs must hold one x per member")
    members = []
    for m in range(M):
        g = graph.clone()
        bc = torch.as_tensor(bcs[m]).to(graph.BC.dtype)
        if bc.shape != graph.BC.shape:
            raise ValueError(f"bcs[{m}] has shape {tuple(bc.shape)}, the graph's BC {tuple(graph.BC.shape)}")
        g.BC = bc
        if xs is not None:
            x = torch.as_tensor(xs[m]).to(graph.x.dtype)
            if x.shape != graph.x.shape:
                raise ValueError(f"xs[{m}] has shape {tuple(x.shape)}, the graph's x {tuple(graph.x.shape)}")
            g.x = x
        members.append(g)
    return adapt_batch_training(collate(members))


def member_ranges(batch):
    """The members' row ranges: ``finest_ranges(batch)``, checked for equal length."""
    ranges = finest_ranges(batch)
    if len({e - s for s, e in ranges}) != 1:
        raise ValueError("the members of an ensemble share one mesh: finest ranges of equal length")
    return ranges


def _members(ranges):
    ranges = [(int(s), int(e)) for s, e in ranges]
    if not 1 <= len(ranges) <= L.MAX_ENSEMBLE_MEMBERS:
        raise ValueError(f"an ensemble has 1..{L.MAX_ENSEMBLE_MEMBERS} members, not {len(ranges)}")
    n = ranges[0][1] - ranges[0][0]
    if n < 0 or any(s < 0 or e - s != n for s, e in ranges):
        raise ValueError("member ranges must start at 0 or later and have equal length")
    return [s for s, _ in ranges], n


def _mean_torch(v):
    """[M, ...] float32 -> the fp64 sum in member order from 0, divided by M, rounded to float32."""
    s = torch.zeros(v.shape[1:], dtype=torch.float64, device=v.device)
    for m in range(v.shape[0]):
        s = s + v[m].double()
    return (s / float(v.shape[0])).float()


def _steps_torch(pred, row0, n, thresholds=(0.05, 0.3)):
    """The per-step statistics of ``pred`` [N, 2, t] across the members at rows ``row0`` from plain
    torch ops, walking the members in order.  Returns every array of STEP_NAMES, ``wet_members`` as
    ``[n_thr, n, t]``."""
    h = torch.stack([pred[r:r + n, 0, :].float() for r in row0])         # [M, n, t]
    out = {"h_mean": _mean_torch(h)}
    mn = torch.full(h.shape[1:], float("inf"), device=h.device)
    mx = -mn
    for m in range(h.shape[0]):
        mn = torch.where(h[m] < mn, h[m], mn)
        mx = torch.where(h[m] > mx, h[m], mx)
    out["h_min"], out["h_max"] = mn, mx
    wet = [(h > thr).sum(0).to(torch.int32) for thr in thresholds]       # strict, float32 against float32
    out["wet_members"] = torch.stack(wet) if wet else torch.zeros((0,) + h.shape[1:], dtype=torch.int32, device=h.device)
    return out


def _maps_torch(values, steps, thresholds, ranks):
    """The cross-member reduction of ``values`` [M, n] float32 and ``steps`` [M, n] int32 (either
    may be None) from plain torch ops: a stable ascending sort along the members, -1 steps after
    every step.  The outputs of ``msw_ensemble_maps_out``, per-threshold and per-rank ones stacked."""
    out = {}
    ranks = torch.as_tensor(list(ranks), dtype=torch.int64)
    if values is not None:
        n = values.shape[1]
        ex = [(values > thr).sum(0).to(torch.int32) for thr in thresholds]
        out["exceed_members"] = torch.stack(ex) if ex else torch.zeros(0, n, dtype=torch.int32, device=values.device)
        out["mean"] = _mean_torch(values)
        out["rank_values"] = torch.sort(values, dim=0, stable=True).values[ranks.to(values.device)]
    if steps is not None:
        out["members_with_step"] = (steps >= 0).sum(0).to(torch.int32)
        key = torch.where(steps < 0, torch.full_like(steps, _INT_MAX), steps)
        sel = torch.sort(key, dim=0, stable=True).values[ranks.to(steps.device)]
        out["rank_steps"] = torch.where(sel == _INT_MAX, torch.full_like(sel, -1), sel)
    return out


def _thr_array(thresholds):
    return (C.c_float * max(len(thresholds), 1))(*thresholds)


def _stream(stream, device):
    return C.c_void_p(stream if stream is not None else torch.cuda.current_stream(device).cuda_stream)


class EnsembleSteps:
    """Per-step statistics across the members at row ranges ``ranges`` (equal length n, member
    order = list order) over ``steps`` steps, filled column by column by successive :meth:`update`
    calls.  ``want``: the arrays to produce (names of STEP_NAMES, default all)."""

    def __init__(self, ranges, steps, thresholds=(0.05, 0.3), want=None, device="cpu"):
        self.row0, self.num_cells = _members(ranges)
        self.num_members = len(self.row0)
        self.steps = int(steps)
        self.thresholds = tuple(float(t) for t in thresholds)
        if len(self.thresholds) > L.MAX_MAP_THRESHOLDS:
            raise ValueError(f"at most {L.MAX_MAP_THRESHOLDS} thresholds")
        self.device = torch.device(device)
        self.want = tuple(STEP_NAMES if want is None else want)
        unknown = set(self.want) - set(STEP_NAMES)
        if unknown:
            raise ValueError(f"unknown arrays {sorted(unknown)}; choose from {STEP_NAMES}")
        self.steps_seen = 0
        n = self.num_cells
        self.arrays = {}
        for k in self.want:  # every update overwrites its columns: no initialisation
            shape = (len(self.thresholds), n, self.steps) if k == "wet_members" else (n, self.steps)
            self.arrays[k] = torch.empty(shape, device=self.device,
                                         dtype=torch.int32 if k == "wet_members" else torch.float32)

    def update(self, pred, t_begin=0, t_count=None, stream=None):
        """Reduce steps ``t_begin .. t_begin + t_count - 1`` of ``pred`` [N, 2, T] (graph
        numbering, N covering every member's rows) into the next ``t_count`` columns."""
        if pred.dim() != 3 or pred.shape[1] != 2:
            raise ValueError("pred must be [N, 2, T]")
        T = int(pred.shape[2])
        t_begin = int(t_begin)
        t_count = T - t_begin if t_count is None else int(t_count)
        if t_begin < 0 or t_count < 0 or t_begin + t_count > T:
            raise ValueError(f"steps [{t_begin}, {t_begin + t_count}) lie outside the rollout's {T}")
        if pred.shape[0] < max(self.row0) + self.num_cells:
            raise ValueError(f"pred has {pred.shape[0]} rows, the members reach row {max(self.row0) + self.num_cells}")
        if pred.device != self.device:
            raise ValueError(f"pred is on {pred.device}, the statistics on {self.device}")
        if self.steps_seen + t_count > self.steps:
            raise ValueError(f"{self.steps_seen} + {t_count} steps exceed the {self.steps} the arrays hold")
        if t_count and self.num_cells:
            if pred.is_cuda:
                self._update_hip(pred, T, t_begin, t_count, stream)
            else:
                new = _steps_torch(pred[:, :, t_begin:t_begin + t_count], self.row0, self.num_cells, self.thresholds)
                for k in self.want:
                    self.arrays[k][..., self.steps_seen:self.steps_seen + t_count] = new[k]
        self.steps_seen += t_count
        return self

    def _update_hip(self, pred, T, t_begin, t_count, stream):
        if pred.dtype != torch.float32 or not pred.is_contiguous():
            pred = pred.float().contiguous()
        out = L.MswEnsembleStepsOut(**{k: self.arrays[k].data_ptr() for k in self.want})
        row0 = (C.c_int64 * self.num_members)(*self.row0)
        L.check(L.lib().msw_ensemble_steps_update(C.c_void_p(pred.data_ptr()), T, t_begin, t_count, row0,
                                                  self.num_members, self.num_cells, _thr_array(self.thresholds),
                                                  len(self.thresholds), self.steps, self.steps_seen, C.byref(out),
                                                  _stream(stream, pred.device)))

    def launch(self, t_count):
        """``(grid, cells_per_wg, iters)`` of the update of a window of ``t_count`` steps."""
        return steps_launch(self.num_cells, self.num_members, t_count)

    def result(self):
        """The statistics of the steps seen so far as a dict: ``h_mean``, ``h_min``, ``h_max``
        [n, steps]; ``wet_members`` (int32) and ``wet_prob`` = wet_members / M (float32) as
        {threshold: [n, steps]}; ``members``; ``steps``."""
        t = self.steps_seen
        out = {"steps": t, "members": self.num_members}
        for k in self.want:
            v = self.arrays[k][..., :t]
            if k == "wet_members":
                out[k] = {thr: v[i] for i, thr in enumerate(self.thresholds)}
                out["wet_prob"] = {thr: w.float() / self.num_members for thr, w in out[k].items()}
            else:
                out[k] = v
        return out


def steps_launch(n, M, t_count):
    """``(grid, cells_per_wg, iters)`` of ``msw_ensemble_steps_update`` for n cells, M members and
    a window of ``t_count`` steps (host only)."""
    g, c, it = C.c_int32(), C.c_int32(), C.c_int32()
    L.check(L.lib().msw_ensemble_steps_launch(int(n), int(M), int(t_count), C.byref(g), C.byref(c), C.byref(it)))
    return g.value, c.value, it.value


def _maps_hip(values, steps, thresholds, ranks, stream):
    src = values if values is not None else steps
    M, n = src.shape
    dev = src.device
    out = {}
    if values is not None:
        out["exceed_members"] = torch.empty(len(thresholds), n, dtype=torch.int32, device=dev)
        out["mean"] = torch.empty(n, dtype=torch.float32, device=dev)
        out["rank_values"] = torch.empty(len(ranks), n, dtype=torch.float32, device=dev)
    if steps is not None:
        out["members_with_step"] = torch.empty(n, dtype=torch.int32, device=dev)
        out["rank_steps"] = torch.empty(len(ranks), n, dtype=torch.int32, device=dev)
    o = L.MswEnsembleMapsOut(**{k: v.data_ptr() for k, v in out.items() if v.numel()})
    rk = (C.c_int32 * max(len(ranks), 1))(*ranks)
    L.check(L.lib().msw_ensemble_maps(C.c_void_p(values.data_ptr() if values is not None else 0),
                                      C.c_void_p(steps.data_ptr() if steps is not None else 0), M, n,
                                      _thr_array(thresholds), len(thresholds), rk, len(ranks), C.byref(o),
                                      _stream(stream, dev)))
    return out


def ensemble_maps(values=None, steps=None, thresholds=(), probs=(0.1, 0.5, 0.9), stream=None):
    """The one-shot reduction across members of per-member maps.  ``values``: [M, n] (e.g. every
    member's ``h_max``) or None; ``steps``: [M, n] integers (e.g. ``first_wet`` at one threshold,
    -1 = never) or None; at most 8 ``probs``.  Returns a dict; from ``values``:
      exceed_members  {threshold: [n] int32}  members with value > threshold (strict)
      exceed_prob     {threshold: [n]}        exceed_members / M
      mean            [n]                     the fp64 sum in member order / M, as float32
      quantiles       {p: [n]}                the value of rank ``quantile_rank(p, M)``, exact
    from ``steps``:
      members_with_step  [n] int32            members with a step >= 0
      step_quantiles     {p: [n] int32}       the first step by which at least rank + 1 members
                                              have one, -1 where fewer have"""
    src = values if values is not None else steps
    if src is None:
        raise ValueError("give values, steps or both")
    if src.dim() != 2 or (values is not None and steps is not None and values.shape != steps.shape):
        raise ValueError("values and steps must be [M, n] of one shape")
    if values is not None and steps is not None and values.device != steps.device:
        raise ValueError("values and steps must be on one device")
    M = int(src.shape[0])
    if not 1 <= M <= L.MAX_ENSEMBLE_MEMBERS:
        raise ValueError(f"an ensemble has 1..{L.MAX_ENSEMBLE_MEMBERS} members, not {M}")
    thresholds = tuple(float(t) for t in thresholds)
    probs = tuple(probs)
    if len(thresholds) > L.MAX_MAP_THRESHOLDS:
        raise ValueError(f"at most {L.MAX_MAP_THRESHOLDS} thresholds")
    if len(probs) > L.MAX_ENSEMBLE_RANKS:
        raise ValueError(f"at most {L.MAX_ENSEMBLE_RANKS} probabilities")
    ranks = [quantile_rank(p, M) for p in probs]
    if values is not None:
        values = values.float().contiguous()
    if steps is not None:
        steps = steps.to(torch.int32).contiguous()
    if src.is_cuda:
        raw = _maps_hip(values, steps, thresholds, ranks, stream) if src.shape[1] else \
            _maps_torch(values, steps, thresholds, ranks)
    else:
        raw = _maps_torch(values, steps, thresholds, ranks)
    out = {"members": M}
    if values is not None:
        out["exceed_members"] = {t: raw["exceed_members"][i] for i, t in enumerate(thresholds)}
        out["exceed_prob"] = {t: v.float() / M for t, v in out["exceed_members"].items()}
        out["mean"] = raw["mean"]
        out["quantiles"] = {p: raw["rank_values"][j] for j, p in enumerate(probs)}
    if steps is not None:
        out["members_with_step"] = raw["members_with_step"]
        out["step_quantiles"] = {p: raw["rank_steps"][j] for j, p in enumerate(probs)}
    return out


class EnsembleMaps:
    """A rollout reduced to ensemble maps: one :class:`FloodMaps` per member (row ranges
    ``ranges``), fed by :meth:`update`, reduced across members by :meth:`result`.  ``of``: the
    per-member maps to reduce -- ``h_max``, ``q_max``, ``vel_max``, ``froude_max`` (exceedance
    at ``thresholds`` for ``h_max`` only) and ``first_wet`` (per threshold)."""

    def __init__(self, ranges, thresholds=(0.05, 0.3), probs=(0.1, 0.5, 0.9), of=("h_max",), device="cpu"):
        self.row0, self.num_cells = _members(ranges)
        self.num_members = len(self.row0)
        self.thresholds = tuple(float(t) for t in thresholds)
        self.probs = tuple(probs)
        self.of = tuple(of)
        unknown = set(self.of) - set(_VALUE_MAPS) - {"first_wet"}
        if unknown:
            raise ValueError(f"unknown maps {sorted(unknown)}; choose from {_VALUE_MAPS + ('first_wet',)}")
        if len(self.probs) > L.MAX_ENSEMBLE_RANKS:
            raise ValueError(f"at most {L.MAX_ENSEMBLE_RANKS} probabilities")
        for p in self.probs:
            quantile_rank(p, self.num_members)
        self.members = [FloodMaps(self.num_cells, r, thresholds=self.thresholds, device=device, want=self.of)
                        for r in self.row0]

    @property
    def steps_seen(self):
        return self.members[0].steps_seen

    def update(self, pred, t_begin=0, t_count=None, stream=None):
        for fm in self.members:
            fm.update(pred, t_begin, t_count, stream)
        return self

    def result(self, temporal_res=None, stream=None):
        """{map: ``ensemble_maps`` of the members' maps stacked to [M, n]} for the value maps,
        ``first_wet``: {threshold: ``ensemble_maps`` of the members' first wet steps}; ``steps``,
        ``members``.  With ``temporal_res`` (minutes per step) every ``first_wet`` entry also has
        ``arrival_hours`` {p: [n]}: the time of its step quantile, NaN where it is -1."""
        if not self.steps_seen:
            raise RuntimeError("no step has been reduced yet")
        out = {"steps": self.steps_seen, "members": self.num_members}
        for k in self.of:
            stack = torch.stack([fm.maps[k] for fm in self.members])
            if k != "first_wet":
                out[k] = ensemble_maps(values=stack, thresholds=self.thresholds if k == "h_max" else (),
                                       probs=self.probs, stream=stream)
                continue
            out[k] = {}
            for i, thr in enumerate(self.thresholds):
                res = ensemble_maps(steps=stack[:, i], probs=self.probs, stream=stream)
                if temporal_res is not None:
                    res["arrival_hours"] = {}
                    for p, s in res["step_quantiles"].items():
                        hours = _over_60(s.long() * temporal_res)
                        res["arrival_hours"][p] = torch.where(s >= 0, hours, torch.full_like(hours, float("nan")))
                out[k][thr] = res
        return out


# ---------------------------------------------------------------------------- scores
_MIN_BLOCK, _BLOCKS, _MAX_BLOCK = 16, 2048, 32768


def _block_cells(n):
    """The cells of a summation block for n cells (csrc/scores.hip ``pick_launch``)."""
    grown = -(-n // (_MIN_BLOCK * _BLOCKS)) * _MIN_BLOCK
    return min(max(grown, _MIN_BLOCK), _MAX_BLOCK)


def _sum_cells(x):
    """[n, t] float64 -> [t]: the kernel's order -- blocks of ``_block_cells(n)`` consecutive
    cells, a block added in cell order from 0, the blocks in block order.  It does not depend on t."""
    n, t = x.shape
    cpb = _block_cells(n)
    nb = -(-n // cpb)
    xb = torch.cat([x, torch.zeros(nb * cpb - n, t, dtype=x.dtype, device=x.device)]).view(nb, cpb, t)
    part = torch.zeros(nb, t, dtype=x.dtype, device=x.device)
    for j in range(cpb):
        part = part + xb[:, j]
    total = torch.zeros(t, dtype=x.dtype, device=x.device)
    for b in range(nb):
        total = total + part[b]
    return total


def _scores_torch(pred, row0, n, truth, thresholds=(0.05, 0.3)):
    """The scores of ``pred`` [N, 2, t] across the members at rows ``row0`` against ``truth``
    [n, t] (float32 depths) from plain torch ops -> ``sums`` [t, 5] float64, ``reliability``
    [t, n_thr, M + 1, 2] int64 and ``crps_terms`` [n, t] float64 (M a - b per cell and step)."""
    h = torch.stack([pred[r:r + n, 0, :].float() for r in row0])          # [M, n, t]
    M, t = h.shape[0], h.shape[2]
    y32 = truth.float()
    hd, y = h.double(), y32.double()
    a, S, Q = torch.zeros_like(y), torch.zeros_like(y), torch.zeros_like(y)
    for m in range(M):                                                    # member order
        a = a + (hd[m] - y).abs()
        S = S + hd[m]
        Q = Q + hd[m] * hd[m]
    asc = torch.sort(h, dim=0).values.double()
    b = torch.zeros_like(y)
    for i in range(M):                                                    # b = sum_i (2 i - M + 1) h_(i), i from 0
        b = b + float(2 * i - M + 1) * asc[i]
    e = S - float(M) * y
    v = float(M) * Q - S * S
    bad = torch.isnan(a)                                                  # a NaN depth: every term is NaN
    b, v = torch.where(bad, a, b), torch.where(bad, a, v)
    sums = torch.stack([_sum_cells(x) for x in (a, b, e.abs(), e * e, v)], dim=1)
    table = torch.zeros(t, len(thresholds), M + 1, 2, dtype=torch.int64, device=h.device)
    col = torch.arange(t, device=h.device)[None, :] * (M + 1)
    for k, thr in enumerate(thresholds):                                  # strict, float32 against float32
        key = ((h > thr).sum(0) + col).reshape(-1)
        obs = (y32 > thr).reshape(-1)
        table[:, k, :, 0] = torch.bincount(key, minlength=t * (M + 1)).view(t, M + 1)
        table[:, k, :, 1] = torch.bincount(key[obs], minlength=t * (M + 1)).view(t, M + 1)
    return {"sums": sums, "reliability": table, "crps_terms": float(M) * a - b}


def scores_launch(n, M, t_count):
    """``(grid, cells_per_wg, iters)`` of ``msw_ensemble_scores_update`` for n cells, M members and
    a window of ``t_count`` steps (host only); ``grid`` depends on n alone."""
    g, c, it = C.c_int32(), C.c_int32(), C.c_int32()
    L.check(L.lib().msw_ensemble_scores_launch(int(n), int(M), int(t_count), C.byref(g), C.byref(c), C.byref(it)))
    return g.value, c.value, it.value


class EnsembleScores:
    """The ensemble at row ranges ``ranges`` (equal length n, member order = list order) scored
    against a truth run over ``steps`` steps, column by column by successive :meth:`update` calls.
    ``want``: what to produce (names of SCORE_NAMES, default all)."""

    def __init__(self, ranges, steps, thresholds=(0.05, 0.3), want=None, device="cpu"):
        self.row0, self.num_cells = _members(ranges)
        self.num_members = len(self.row0)
        self.steps = int(steps)
        self.thresholds = tuple(float(t) for t in thresholds)
        if len(self.thresholds) > L.MAX_MAP_THRESHOLDS:
            raise ValueError(f"at most {L.MAX_MAP_THRESHOLDS} thresholds")
        self.device = torch.device(device)
        self.want = tuple(SCORE_NAMES if want is None else want)
        unknown = set(self.want) - set(SCORE_NAMES)
        if unknown:
            raise ValueError(f"unknown scores {sorted(unknown)}; choose from {SCORE_NAMES}")
        self.steps_seen = 0
        n, M = self.num_cells, self.num_members
        self.arrays = {}
        if "sums" in self.want:          # every update overwrites its columns: no initialisation
            self.arrays["sums"] = torch.empty(self.steps, len(SCORE_SUMS), dtype=torch.float64, device=self.device)
        if "reliability" in self.want:
            self.arrays["reliability"] = torch.empty(self.steps, len(self.thresholds), M + 1, 2, dtype=torch.int64,
                                                     device=self.device)
        if "cell_crps" in self.want:     # carried from call to call
            self.arrays["cell_crps"] = torch.zeros(n, dtype=torch.float64, device=self.device)

    def update(self, pred, truth, t_begin=0, t_count=None, truth_row0=0, truth_t0=None, stream=None):
        """Score steps ``t_begin .. t_begin + t_count - 1`` of ``pred`` [N, 2, T] against columns
        ``truth_t0 ..`` (default: the steps seen so far -- a truth that holds the whole horizon) of
        rows ``truth_row0 .. truth_row0 + n - 1`` of ``truth`` [rows, 2, T_truth], into the next
        ``t_count`` columns.  ``truth`` may be ``pred`` itself."""
        if pred.dim() != 3 or pred.shape[1] != 2:
            raise ValueError("pred must be [N, 2, T]")
        if truth.dim() != 3 or truth.shape[1] != 2:
            raise ValueError("truth must be [rows, 2, T_truth]")
        T, Tt = int(pred.shape[2]), int(truth.shape[2])
        t_begin, truth_row0 = int(t_begin), int(truth_row0)
        t_count = T - t_begin if t_count is None else int(t_count)
        truth_t0 = self.steps_seen if truth_t0 is None else int(truth_t0)
        if t_begin < 0 or t_count < 0 or t_begin + t_count > T:
            raise ValueError(f"steps [{t_begin}, {t_begin + t_count}) lie outside the rollout's {T}")
        if truth_t0 < 0 or truth_t0 + t_count > Tt:
            raise ValueError(f"truth columns [{truth_t0}, {truth_t0 + t_count}) lie outside the truth's {Tt}")
        if pred.shape[0] < max(self.row0) + self.num_cells:
            raise ValueError(f"pred has {pred.shape[0]} rows, the members reach row {max(self.row0) + self.num_cells}")
        if truth_row0 < 0 or truth.shape[0] < truth_row0 + self.num_cells:
            raise ValueError(f"truth has {truth.shape[0]} rows, the cells reach row {truth_row0 + self.num_cells}")
        if pred.device != self.device or truth.device != self.device:
            raise ValueError(f"pred is on {pred.device}, truth on {truth.device}, the scores on {self.device}")
        if self.steps_seen + t_count > self.steps:
            raise ValueError(f"{self.steps_seen} + {t_count} steps exceed the {self.steps} the arrays hold")
        if t_count and self.num_cells and self.arrays:
            if pred.is_cuda:
                self._update_hip(pred, truth, T, Tt, t_begin, t_count, truth_row0, truth_t0, stream)
            else:
                n, at = self.num_cells, self.steps_seen
                new = _scores_torch(pred[:, :, t_begin:t_begin + t_count], self.row0, n,
                                    truth[truth_row0:truth_row0 + n, 0, truth_t0:truth_t0 + t_count], self.thresholds)
                for k in ("sums", "reliability"):
                    if k in self.arrays:
                        self.arrays[k][at:at + t_count] = new[k]
                if "cell_crps" in self.arrays:
                    for t in range(t_count):     # one addition per step, in step order, onto the carried value
                        self.arrays["cell_crps"] += new["crps_terms"][:, t]
        self.steps_seen += t_count
        return self

    def _update_hip(self, pred, truth, T, Tt, t_begin, t_count, truth_row0, truth_t0, stream):
        same = truth is pred
        if pred.dtype != torch.float32 or not pred.is_contiguous():
            pred = pred.float().contiguous()
        if same:
            truth = pred
        elif truth.dtype != torch.float32 or not truth.is_contiguous():
            truth = truth.float().contiguous()
        out = L.MswEnsembleScoresOut(**{k: v.data_ptr() for k, v in self.arrays.items() if v.numel()})
        row0 = (C.c_int64 * self.num_members)(*self.row0)
        L.check(L.lib().msw_ensemble_scores_update(C.c_void_p(pred.data_ptr()), T, t_begin, t_count, row0,
                                                   self.num_members, self.num_cells, C.c_void_p(truth.data_ptr()),
                                                   Tt, truth_t0, truth_row0, _thr_array(self.thresholds),
                                                   len(self.thresholds), self.steps, self.steps_seen, C.byref(out),
                                                   _stream(stream, pred.device)))

    def launch(self, t_count):
        """``(grid, cells_per_wg, iters)`` of the update of a window of ``t_count`` steps."""
        return scores_launch(self.num_cells, self.num_members, t_count)

    def result(self):
        """The scores of the steps seen so far as a dict (float64 throughout).  From ``sums``
        [steps, 5] = the sums over the cells of a, b, |e|, e^2, v:
          crps [steps] = sum a / (M n) - sum b / (M^2 n), ``crps_mean`` its mean over the steps
          mae_mean     = sum |e| / (M n)            the ensemble mean's absolute error
          rmse_mean    = sqrt(sum e^2 / (M^2 n))    ... and its RMSE
          spread       = sqrt(sum v / (M^2 n))      the root of the mean population variance
          spread_skill = spread / rmse_mean
        from the table: ``reliability`` {thr: {forecast_prob [M + 1] = c / M, n [steps, M + 1] the
        cells forecast c / M, observed [steps, M + 1] those of them above thr}} and ``brier``
        {thr: [steps]} = the mean of (c / M - o)^2; ``cell_crps`` [n] = the time-mean CRPS map;
        ``members``, ``steps``."""
        t, M, n = self.steps_seen, self.num_members, self.num_cells
        out = {"steps": t, "members": M}
        if "sums" in self.arrays:
            s = self.arrays["sums"][:t]
            out["sums"] = s
            out["crps"] = s[:, 0] / (M * n) - s[:, 1] / (M * M * n)
            out["crps_mean"] = out["crps"].mean() if t else out["crps"].sum()
            out["mae_mean"] = s[:, 2] / (M * n)
            out["rmse_mean"] = torch.sqrt(s[:, 3] / (M * M * n))
            out["spread"] = torch.sqrt(s[:, 4] / (M * M * n))
            out["spread_skill"] = out["spread"] / out["rmse_mean"]
        if "reliability" in self.arrays:
            tab = self.arrays["reliability"][:t]
            p = torch.arange(M + 1, dtype=torch.float64, device=self.device) / M
            out["reliability"], out["brier"] = {}, {}
            for k, thr in enumerate(self.thresholds):
                cells, obs = tab[:, k, :, 0], tab[:, k, :, 1]
                out["reliability"][thr] = {"forecast_prob": p, "n": cells, "observed": obs}
                # (p - 1)^2 on the observed cells, p^2 on the others
                out["brier"][thr] = (cells.double() * p * p - 2.0 * p * obs.double() + obs.double()).sum(1) / n
        if "cell_crps" in self.arrays:
            out["cell_crps"] = self.arrays["cell_crps"] / (M * M * max(t, 1))
        return out


def ensemble_scores(pred, truth, ranges, thresholds=(0.05, 0.3), want=None, t_begin=0, t_count=None, truth_row0=0,
                    truth_t0=0, stream=None):
    """:class:`EnsembleScores` in one shot: steps ``t_begin .. t_begin + t_count - 1`` (default:
    to the end) of ``pred`` [N, 2, T] against ``truth`` -> ``EnsembleScores.result()``."""
    t_count = int(pred.shape[2]) - int(t_begin) if t_count is None else int(t_count)
    sc = EnsembleScores(ranges, max(t_count, 0), thresholds, want=want, device=pred.device)
    return sc.update(pred, truth, t_begin, t_count, truth_row0, truth_t0, stream).result()


def rollout_ensemble(model, batch, steps=None, chunk=16, thresholds=(0.05, 0.3), probs=(0.1, 0.5, 0.9),
                     per_step=True, keep_rollout=False, of=("h_max", "first_wet"), temporal_res=None, truth=None,
                     truth_row0=0):
    """Roll out the ensemble ``batch`` (:func:`make_ensemble`) ``chunk`` steps at a time
    (``rollout_chunks``; ``chunk=None``: one ``model.rollout``) and feed every piece to an
    :class:`EnsembleMaps` and, with ``per_step``, an :class:`EnsembleSteps`: never more than one
    piece is held.  Returns ``{"maps": EnsembleMaps.result, "steps": EnsembleSteps.result or
    None}``; ``keep_rollout=True`` returns ``(that, rollout)`` with the pieces concatenated (tests).
    With ``truth`` [rows, 2, >= steps] (the cells at rows ``truth_row0 ..``) every piece also feeds
    an :class:`EnsembleScores`, whose result is added as ``"scores"``."""
    T = int(batch.y.shape[-1] if steps is None else steps)
    ranges = member_ranges(batch)
    dev = batch.x.device
    em = EnsembleMaps(ranges, thresholds, probs, of=of, device=dev)
    es = EnsembleSteps(ranges, T, thresholds, device=dev) if per_step else None
    sc = EnsembleScores(ranges, T, thresholds, device=dev) if truth is not None else None
    kept = []
    pieces = [(0, model.rollout(batch, T))] if chunk is None else rollout_chunks(model, batch, T, chunk)
    for _, pred in pieces:
        em.update(pred)
        if es is not None:
            es.update(pred)
        if sc is not None:
            sc.update(pred, truth, truth_row0=truth_row0)
        if keep_rollout:
            kept.append(pred)
    out = {"maps": em.result(temporal_res), "steps": es.result() if es is not None else None}
    if sc is not None:
        out["scores"] = sc.result()
    return (out, torch.cat(kept, -1)) if keep_rollout else out
