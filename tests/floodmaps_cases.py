"""The flood-map kernel (msw_flood_maps_update, csrc/floodmaps.hip) as test cases: the windows that
reach every staging geometry with every loader, rollouts with rows planted from that geometry, and
a part-by-part restatement of the maps with wrong variants, each a plausible kernel error.

A plain module (no test in it), shared by tests/test_floodmaps.py (CPU: the census of the launch
query, the restatement against ``_maps_torch``, every variant caught in every class) and
tests/test_gpu_floodmaps.py (the kernel against ``_maps_torch``).

Geometry.  A launch takes at most 1024 steps (longer windows run as carried-over slabs) and stages
R rows per round, R = ``rows_per_wg`` of the launch query: 32 rows up to 32 steps, halved at 33, 66,
132, 264 and 528 steps.  The 64 lanes reduce a round as R rows x P = 64 / R consecutive time parts
of tp = ceil(tc / P) steps, trailing parts may be empty (tc = 132: 16 parts of 9 steps, the last
one empty), and the parts are merged in time order.  The 16-byte loader takes a whole window of an
even T from a 16-byte aligned base; everything else goes through the scalar loader.
"""
import ctypes as C

import torch

from mswegnn import _lib
from mswegnn.floodmaps import MAP_NAMES, _maps_torch

THR4 = (0.05, 0.3, 0.0, 1.0)
EPS = 0.01
SLAB = 1024          # steps of one launch at most (csrc/floodmaps.hip kMaxTc)
T_OFFSET = 11        # global step of a window's first column in the sweep


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


# ------------------------------------------------------------------ the launch geometry
def rows_per_wg(tc):
    g, r, it = C.c_int32(), C.c_int32(), C.c_int32()
    _lib.check(_lib.lib().msw_flood_maps_launch(1000, int(tc), C.byref(g), C.byref(r), C.byref(it)))
    return r.value


def slabs(t_count):
    """[(first step, steps)] of the launches of a window, in window coordinates."""
    return [(s0, min(SLAB, t_count - s0)) for s0 in range(0, t_count, SLAB)]


def part_starts(t_count):
    """First steps (window coordinates, ascending) of the non-empty time parts of every launch of
    a window of ``t_count`` steps, from the geometry the launch query reports."""
    out = []
    for s0, tc in slabs(t_count):
        P = 64 // rows_per_wg(tc)
        tp = -(-tc // P)
        out += [s0 + k * tp for k in range(P) if k * tp < tc]
    return out


# ------------------------------------------------------------------ the windows
class Case:
    """A window [t_begin, t_begin + t_count) of rows of T steps whose first row sits ``shift``
    floats past a 16-byte aligned address."""

    def __init__(self, T, t_begin, t_count, shift=0):
        self.T, self.t_begin, self.t_count, self.shift = T, t_begin, t_count, shift

    @property
    def vec(self):
        """The whole window takes the 16-byte loader (only a one-launch window can)."""
        return self.t_begin == 0 and self.t_count == self.T and self.T % 2 == 0 and self.shift % 4 == 0

    @property
    def id(self):
        return f"T{self.T}-b{self.t_begin}-c{self.t_count}" + (f"-shift{self.shift}" if self.shift else "")

    def launches(self):
        """[(steps, rows per round, 16-byte loader)] of the window's launches."""
        return [(tc, rows_per_wg(tc), self.vec) for _, tc in slabs(self.t_count)]

    def row_counts(self):
        """nrows around every rows-per-round of the window's launches, plus one count that holds
        every planted row."""
        n = {PERIOD}
        for _, R, _ in self.launches():
            n |= {1, R - 1, R, R + 1, 2 * R + 1}
        return sorted(n - {0})


VEC_T = (32, 34, 64, 66, 100, 130, 132, 200, 262, 264, 400, 526, 528, 1024)
SCALAR_TC = (31, 33, 65, 66, 131, 132, 263, 264, 527, 528, 1024)
SHIFTED_T = (32, 64, 66, 132, 264, 528)     # one per class, even T from a base shifted by one float

CASES = [Case(T, 0, T) for T in VEC_T]
CASES += [Case(tc | 1, 0, tc) for tc in SCALAR_TC]                 # an odd T
CASES += [Case(tc + 8, 3, tc) for tc in SCALAR_TC]                 # a window of a longer row
CASES += [Case(T, 0, T, shift=1) for T in SHIFTED_T]
CASES += [Case(1025, 0, 1025), Case(2049, 0, 2049), Case(1040, 5, 1030)]   # slabs: 1024 + 1, 1024 + 1024 + 1, 1024 + 6

# one class each of R = 4, 2, 1: (T, pieces).  The one-shot parts are 13 steps long at T = 200 and
# 400 and 16 steps at T = 1100 (its first launch), so the cuts 6 | 7 fall inside a part, 26 and 512
# on a part boundary, and 1024 / 1030 at and past the slab boundary.
CARRY = [(200, (6, 20, 174)), (400, (6, 20, 200, 174)), (1100, (7, 505, 512, 76)), (1100, (1030, 70))]


# ------------------------------------------------------------------ the rollouts
def make_rollout(n, T, seed):
    """[n, 2, T] seeded values on a 2^-12 grid (no denormals anywhere, also not in q / h), with
    planted rows, cycling over the row index: never wet; always wet; wet - dry - wet; the maximum
    of h and of |q| tied at two steps (q with opposite signs); h exactly at the thresholds, at
    vel_eps and at 0; 0 < h < vel_eps throughout; two plain random rows."""
    gen = torch.Generator().manual_seed(seed)
    h = torch.round(torch.rand(n, T, generator=gen) * 1.5 * 4096) / 4096
    h = torch.where(torch.rand(n, T, generator=gen) < 0.45, torch.zeros(()), h)
    q = torch.round((torch.rand(n, T, generator=gen) * 2 - 1) * 4096) / 4096   # negative discharges too
    q = torch.where(torch.rand(n, T, generator=gen) < 0.2, torch.zeros(()), q)
    kind = torch.arange(n) % 8
    t = torch.arange(T)
    h[kind == 0] = 0.0
    q[kind == 0] = 0.0
    h[kind == 1] += 0.5
    third = max(T // 3, 1)
    mid = (t >= third) & (t < T - third)
    h[kind == 2] = torch.where(mid, torch.zeros(()), h[kind == 2] + 0.25)
    t1, t2 = (T // 4) % T, (T - 1 - T // 5) % T
    for tt, sign in ((t1, -1.0), (t2, 1.0)):
        h[kind == 3, tt] = 3.0
        q[kind == 3, tt] = sign * 2.0
    for i, v in enumerate((f32(0.05), f32(0.3), f32(EPS), 0.0, 1.0)):
        h[kind == 4, i % T] = v
    h[kind == 5] = 0.005
    q[kind == 5] = 0.75
    return torch.stack((h, q), 1).contiguous()


N_PLANTED = 12
PERIOD = 8 + N_PLANTED   # rows i with i % PERIOD < 8 keep make_rollout's kinds, the others are planted


def planted_rollout(n, T, t_begin, t_count, seed):
    """``make_rollout`` with, at rows i % PERIOD = 8 + j, the rows planted from the geometry of the
    window [t_begin, t_begin + t_count) (steps below count from the window's first; the window
    needs at least 5 steps and two parts).  Every value outside a plant stays below 2 (h) and at
    most 1 (|q|); a tie is h = 3 at both steps and q = -2 then +2.
      0, 1, 2  ties straddling the first, a middle and the last boundary between non-empty parts
      3   a tie at steps 0 and t_count - 1
      4   the maximum in the middle of the last non-empty part only
      5   a constant row (its maximum step is the first step)
      6   wet up to a part boundary, dry for one whole part, wet again (two parts: wet, then dry)
      7   the maximum at the last step only (t_count = 132: step 131, the last part is empty)
      8   a tie at steps 1023 | 1024 (the slab boundary); in a one-launch window at steps 1 | 2, inside a part
      9   first wet at step 1024; in a one-launch window at the first part boundary
      10  a tie at steps 2047 | 2048; in a shorter window at step 0 and the first part boundary
      11  h exactly at vel_eps with the row's largest q / h, then at each threshold, around a
          middle part boundary, the row otherwise wet above every threshold but 1.0."""
    r = make_rollout(n, T, seed)
    w = r[:, :, t_begin:t_begin + t_count]          # a view: plants land in r
    h, q = w[:, 0, :], w[:, 1, :]
    starts = part_starts(t_count)
    assert t_count >= 5 and len(starts) >= 2
    bounds = starts[1:]
    ends = bounds + [t_count]
    rows = torch.arange(n) % PERIOD

    def tie(j, a, b):
        assert 0 <= a < b < t_count
        sel = rows == 8 + j
        h[sel, a] = h[sel, b] = 3.0
        q[sel, a], q[sel, b] = -2.0, 2.0

    tie(0, bounds[0] - 1, bounds[0])
    tie(1, bounds[len(bounds) // 2] - 1, bounds[len(bounds) // 2])
    tie(2, bounds[-1] - 1, bounds[-1])
    tie(3, 0, t_count - 1)
    sel = rows == 8 + 4
    peak = starts[-1] + (t_count - starts[-1]) // 2
    h[sel, peak], q[sel, peak] = 3.0, -2.0
    sel = rows == 8 + 5
    h[sel], q[sel] = 0.75, -0.5
    sel = rows == 8 + 6
    m = len(starts) // 2
    h[sel] += 0.25
    h[sel, starts[m]:ends[m]] = 0.0
    sel = rows == 8 + 7
    h[sel, t_count - 1], q[sel, t_count - 1] = 3.0, 2.0
    if t_count > SLAB:
        tie(8, SLAB - 1, SLAB)
    else:
        tie(8, 1, 2)
    sel = rows == 8 + 9
    first = SLAB if t_count > SLAB else bounds[0]
    h[sel] += 0.25
    h[sel, :first] = 0.0
    if t_count > 2 * SLAB:
        tie(10, 2 * SLAB - 1, 2 * SLAB)
    else:
        tie(10, 0, bounds[0])
    sel = rows == 8 + 11
    h[sel] += 0.5
    b = min(max(bounds[len(bounds) // 2], 2), t_count - 3)
    for i, v in enumerate((f32(EPS), f32(0.05), f32(0.3), 0.0, 1.0)):
        h[sel, b - 2 + i] = v
    q[sel, b - 2] = -1.5
    return r


def case_rollout(case, n):
    return planted_rollout(n, case.T, case.t_begin, case.t_count, seed=case.T + case.t_begin)


# ------------------------------------------------------------------ the restatement, part by part
VARIANTS = ("tie_latest", "thr_ge", "eps_ge", "signed_q", "first_wet_overwritten", "parts_reversed")


def _elementwise(rows, eps, variant):
    """h, |q|, velocity and Froude number of every (row, step), with ``_maps_torch``'s expressions
    on the whole array (so that both round alike)."""
    h = rows[:, 0, :]
    q = rows[:, 1, :] if variant == "signed_q" else rows[:, 1, :].abs()
    vel = q / h
    vel[(h < eps) if variant == "eps_ge" else (h <= eps)] = 0
    fr = vel / torch.sqrt(9.81 * h)
    fr[h <= 0] = 0
    return h, q, vel, fr


def _part_maps(h, q, vel, fr, thr, t0, variant):
    """The maps of one part [n, t] whose first step is global step ``t0``."""
    steps = torch.arange(h.shape[1], dtype=torch.int32) + t0
    big = torch.iinfo(torch.int32).max

    def first(mask):
        return torch.where(mask, steps, torch.full_like(steps, big)).amin(1)

    def last(mask):
        return torch.where(mask, steps, torch.full_like(steps, -1)).amax(1)

    where_max = last if variant == "tie_latest" else first
    out = {"h_max": h.max(1).values, "q_max": q.max(1).values}
    out["t_h_max"] = where_max(h == out["h_max"][:, None])
    out["t_q_max"] = where_max(q == out["q_max"][:, None])
    out["vel_max"], out["froude_max"] = vel.max(1).values, fr.max(1).values
    wet = [(h >= t) if variant == "thr_ge" else (h > t) for t in thr]
    empty = torch.zeros(0, h.shape[0], dtype=torch.int32)
    out["wet_steps"] = torch.stack([w.sum(1).to(torch.int32) for w in wet]) if wet else empty
    f = torch.stack([first(w) for w in wet]) if wet else empty
    out["first_wet"] = torch.where(f == big, torch.full_like(f, -1), f)
    out["last_wet"] = torch.stack([last(w) for w in wet]) if wet else empty
    return out


def _merge(old, new, variant):
    """``new`` follows ``old`` in time: a maximum moves only to a strictly larger value."""
    out = {}
    for v, t in (("h_max", "t_h_max"), ("q_max", "t_q_max")):
        later = (new[v] >= old[v]) if variant == "tie_latest" else (new[v] > old[v])
        out[v] = torch.where(later, new[v], old[v])
        out[t] = torch.where(later, new[t], old[t])
    for v in ("vel_max", "froude_max"):
        out[v] = torch.maximum(old[v], new[v])
    out["wet_steps"] = old["wet_steps"] + new["wet_steps"]
    keep = (new["first_wet"] < 0) if variant == "first_wet_overwritten" else (old["first_wet"] >= 0)
    out["first_wet"] = torch.where(keep, old["first_wet"], new["first_wet"])
    out["last_wet"] = torch.maximum(old["last_wet"], new["last_wet"])
    return out


def maps_by_parts(rows, thr, eps, t_offset, starts, variant=None):
    """The maps of ``rows`` [n, 2, t] reduced part by part (parts begin at ``starts``) and merged
    in time order: what the kernel does.  Without a variant equal to ``_maps_torch`` for any
    ``starts``; each variant is one wrong rule."""
    ends = list(starts[1:]) + [rows.shape[2]]
    arrays = _elementwise(rows, eps, variant)
    parts = [_part_maps(*(v[:, a:b] for v in arrays), thr, t_offset + a, variant) for a, b in zip(starts, ends)]
    if variant == "parts_reversed":
        parts.reverse()
    out = parts[0]
    for p in parts[1:]:
        out = _merge(out, p, variant)
    return out


def changed_maps(a, b):
    return [k for k in MAP_NAMES if not torch.equal(a[k], b[k])]


def yardstick(rows, thr=THR4, t_offset=T_OFFSET):
    return _maps_torch(rows, thr, EPS, t_offset)
