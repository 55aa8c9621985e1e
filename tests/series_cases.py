"""The zone-series kernel (msw_zone_series_update, csrc/series.hip) as test cases: an order-exact
restatement of its sums, data on which the order of additions shows, and the zone sets that make
the kernel cut a window into several launches.

A plain module (no test in it), shared by tests/test_series.py (CPU: the restatement against
``_series_torch``, the order-sensitivity of the data, the census of the steps per launch) and
tests/test_gpu_series.py (the kernel against the restatement, bit for bit).  numpy only, plus the
``Zones`` constructors.

The order (include/mswegnn.h): a zone's row list is cut into chunks of 256 consecutive entries;
a chunk is summed in list order starting from 0.0; a zone of one chunk is that sum, a longer zone is
0.0 plus its chunk sums in chunk order.  Every term is exact in fp64 (a float, or the product of two
floats), so a sum is determined by the order alone and the kernel must reproduce it bit for bit.

The steps per launch S (csrc/series.hip): 1024, or, once the multi-chunk zones of a set hold more
than 512 chunks ("slots"), the whole tiles of 64 steps that 32 MiB of partials hold at 64 bytes per
(slot, step), and 64 at least: 4096 slots -> 128 steps, 4097 slots -> 64.
"""
import numpy as np
import torch

from mswegnn.series import Zones

CHUNK = 256
THR4 = (0.05, 0.3, 0.0, 1.0)
SIZES = (1, 15, 0, 16, 17, 33, 500, 255, 256, 257, 0)   # around a round (16) and a chunk (256); the last is empty
N_SLAB = 300                                            # rows of the multi-launch cases
BIG = 4096 * CHUNK                                      # list entries of the zone that shrinks S to 128


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


# ------------------------------------------------------------------ grid data: every order of additions is exact
def make_pred(n, T, seed):
    """[n, 2, T] seeded values on a 2^-12 grid, 45 % of the depths exactly 0, every fifth row
    cycling through depths exactly at the thresholds; discharges of both signs."""
    gen = torch.Generator().manual_seed(seed)
    h = torch.round(torch.rand(n, T, generator=gen) * 1.5 * 4096) / 4096
    h = torch.where(torch.rand(n, T, generator=gen) < 0.45, torch.zeros(()), h)
    q = torch.round((torch.rand(n, T, generator=gen) * 2 - 1) * 4096) / 4096
    at = torch.tensor([f32(0.05), f32(0.3), 0.0, 1.0])
    h[1::5] = at[(torch.arange(T)[None, :] + torch.arange(h[1::5].shape[0])[:, None]) % 4]
    return torch.stack((h, q), 1).contiguous()


def make_area(n, seed):
    return torch.rand(n, generator=torch.Generator().manual_seed(seed)) * 90 + 10


# ------------------------------------------------------------------ order-sensitive data
def make_pred_wide(n, T, seed):
    """[n, 2, T] float32 with full mantissas: depths log-uniform over 2^-20 .. 16, 10 % of them
    exactly 0 and 10 % exactly at one of THR4; discharges log-uniform over 1e-6 .. 10 in
    magnitude, of both signs, 10 % exactly 0."""
    rng = np.random.RandomState(seed)
    h = np.exp(rng.uniform(np.log(2.0 ** -20), np.log(16.0), (n, T))).astype(np.float32)
    u = rng.uniform(size=(n, T))
    h[u < 0.1] = 0.0
    at = np.array(THR4, np.float32)[rng.randint(0, 4, (n, T))]
    h = np.where((u >= 0.1) & (u < 0.2), at, h)
    q = np.exp(rng.uniform(np.log(1e-6), np.log(10.0), (n, T))).astype(np.float32)
    q *= np.where(rng.uniform(size=(n, T)) < 0.5, -1, 1).astype(np.float32)
    q[rng.uniform(size=(n, T)) < 0.1] = 0.0
    return torch.from_numpy(np.ascontiguousarray(np.stack((h, q), 1), dtype=np.float32))


def make_area_wide(n, seed, lo=1.0, hi=1e4):
    """[n] float32 areas with full mantissas, log-uniform over lo .. hi.  Over 1 .. 1e4 a sum of
    fewer than 2^16 areas is still exact in any order (multiples of 2^-23 below 2^30), so there
    only the volume shows the order; ``wet_area`` shows it with AREA_SPAN."""
    rng = np.random.RandomState(seed)
    return torch.from_numpy(np.exp(rng.uniform(np.log(lo), np.log(hi), n)).astype(np.float32))


AREA_SPAN = dict(lo=1.0, hi=1e11)      # areas whose sums round: the order of wet_area's additions shows


def wetness(pred, thr):
    """pred with its depths replaced by 1.0 where h > thr and 0.0 elsewhere: its volume is the
    wet_area of pred at thr, term by term."""
    out = pred.clone()
    out[:, 0, :] = (pred[:, 0, :] > thr).float()
    return out


# ------------------------------------------------------------------ the restatement
def _np(a, dtype=None):
    a = a.numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a if dtype is None else a.astype(dtype, copy=False)


def _chunks(ptr):
    """-> (zone, first entry, entries) of every chunk; an empty zone has one chunk of 0 entries."""
    zone, off, cnt = [], [], []
    for z in range(len(ptr) - 1):
        m = int(ptr[z + 1] - ptr[z])
        for c in range(max(-(-m // CHUNK), 1)):
            zone.append(z)
            off.append(int(ptr[z]) + c * CHUNK)
            cnt.append(min(CHUNK, m - c * CHUNK))
    return np.array(zone), np.array(off, np.int64), np.array(cnt)


def series_exact(pred, ptr, rows, area=None, thresholds=(), combine="forward"):
    """``volume`` [Z, T] and ``wet_area`` [n_thr, Z, T] of pred [N, 2, T] in the documented order,
    float64: vectorised over steps and chunks, never over list positions.  ``combine``: the order
    in which a multi-chunk zone's chunk sums are added ("reversed" is a wrong variant)."""
    pred, ptr, rows = _np(pred, np.float32), _np(ptr, np.int64), _np(rows, np.int64)
    a = np.ones(pred.shape[0], np.float64) if area is None else _np(area, np.float32).astype(np.float64)
    thr = [np.float32(t) for t in thresholds]
    Z, T = len(ptr) - 1, pred.shape[2]
    zone, off, cnt = _chunks(ptr)
    h = pred[:, 0, :]
    terms = np.stack([a[:, None] * h.astype(np.float64)] + [np.where(h > t, a[:, None], 0.0) for t in thr], 1)
    acc = np.zeros((len(zone), 1 + len(thr), T))   # every term [N, 1 + n_thr, T] is exact
    for j in range(CHUNK):                         # list position j of every chunk that has one
        live = np.nonzero(cnt > j)[0]
        if live.size == 0:
            break
        acc[live] += terms[rows[off[live] + j]]
    out = np.zeros((Z, 1 + len(thr), T))
    first = np.concatenate(([True], zone[1:] != zone[:-1]))
    starts = np.nonzero(first)[0]
    n_chunks = np.diff(np.append(starts, len(zone)))
    for z, c0, n in zip(zone[starts], starts, n_chunks):
        if n == 1:
            out[z] = acc[c0]
            continue
        order = range(c0, c0 + n) if combine == "forward" else range(c0 + n - 1, c0 - 1, -1)
        s = np.zeros((1 + len(thr), T))
        for c in order:
            s += acc[c]
        out[z] = s
    out = np.ascontiguousarray(out.transpose(1, 0, 2))
    return {"volume": out[0], "wet_area": out[1:]}


def series_ref(pred, zones, area=None, thresholds=()):
    """Every series of SERIES_NAMES as torch tensors: ``volume`` and ``wet_area`` from
    ``series_exact``; ``wet_cells``, ``h_max`` and ``q_max``, which no order can change, from how
    often a zone lists each row (so that a zone of a million entries costs no more than its
    distinct rows)."""
    p = _np(pred, np.float32)
    ptr, rows = _np(zones.ptr, np.int64), _np(zones.rows, np.int64)
    Z, T = len(ptr) - 1, p.shape[2]
    out = series_exact(p, ptr, rows, area, thresholds)
    cells = np.zeros((len(thresholds), Z, T), np.int64)
    h_max, q_max = np.zeros((Z, T), np.float32), np.zeros((Z, T), np.float32)
    for z in range(Z):
        r, mult = np.unique(rows[ptr[z]:ptr[z + 1]], return_counts=True)
        if r.size == 0:
            continue                                # an empty zone keeps its zeros
        h = p[r, 0, :]
        h_max[z], q_max[z] = h.max(0), np.abs(p[r, 1, :]).max(0)
        for k, t in enumerate(thresholds):
            cells[k, z] = (mult[:, None] * (h > np.float32(t))).sum(0)
    res = {k: torch.from_numpy(v) for k, v in out.items()}
    res["wet_cells"] = torch.from_numpy(cells.astype(np.int32))
    res["h_max"], res["q_max"] = torch.from_numpy(h_max), torch.from_numpy(q_max)
    return res


# ------------------------------------------------------------------ other orders of the same terms
def _zone_terms(pred, ptr, rows, area, z):
    a = np.ones(pred.shape[0], np.float64) if area is None else _np(area, np.float32).astype(np.float64)
    r = _np(rows, np.int64)[int(ptr[z]):int(ptr[z + 1])]
    return a[r][:, None] * _np(pred, np.float32)[r, 0, :].astype(np.float64)      # [m, T], each exact


def volume_reversed(pred, ptr, rows, area, z):
    """Zone z's volume with its list reversed (then chunked and summed as documented)."""
    r = _np(rows, np.int64)[int(ptr[z]):int(ptr[z + 1])][::-1]
    return series_exact(pred, np.array([0, len(r)]), r, area)["volume"][0]


def volume_pairwise(pred, ptr, rows, area, z):
    """Zone z's volume as a balanced tree over the list (neighbours first)."""
    t = _zone_terms(pred, ptr, rows, area, z)
    while t.shape[0] > 1:
        if t.shape[0] % 2:
            t = np.concatenate((t, np.zeros((1, t.shape[1]))))
        t = t[0::2] + t[1::2]
    return t[0]


def volume_chunks_reversed(pred, ptr, rows, area, z):
    """Zone z's volume with the chunk sums added last chunk first."""
    r = _np(rows, np.int64)[int(ptr[z]):int(ptr[z + 1])]
    return series_exact(pred, np.array([0, len(r)]), r, area, combine="reversed")["volume"][0]


def differing_fraction(a, b):
    """Fraction of the steps at which two series differ."""
    return float(np.mean(np.asarray(a) != np.asarray(b)))


# ------------------------------------------------------------------ the zone sets
def sweep_zones(n, seed):
    """Zones of SIZES entries drawn with replacement from about 70 % of the rows: unsorted,
    duplicated, overlapping.  -> (zones, mask of the rows that no zone lists)."""
    gen = torch.Generator().manual_seed(seed)
    allowed = torch.nonzero(torch.rand(n, generator=gen) < 0.7).flatten()
    if allowed.numel() == 0:
        allowed = torch.zeros(1, dtype=torch.int64)
    lists = [allowed[torch.randint(0, allowed.numel(), (s,), generator=gen)] for s in SIZES]
    unlisted = torch.ones(n, dtype=torch.bool)
    unlisted[torch.cat(lists)] = False
    return Zones.from_lists(lists, n), unlisted


def permutation_zone(n, seed=1):
    return Zones.from_lists([torch.randperm(n, generator=torch.Generator().manual_seed(seed))], n)


def default_slab_zones():
    """S = 1024: the sweep's zones, a permutation of all N_SLAB rows and a zone of four chunks (two
    chunk sums commute: only three or more show the order in which they are added)."""
    four = torch.randint(0, N_SLAB, (3 * CHUNK + 5,), generator=torch.Generator().manual_seed(32))
    return sweep_zones(N_SLAB, seed=31)[0] + permutation_zone(N_SLAB) + Zones.from_lists([four], N_SLAB)


def big_zones(extra=0):
    """One zone of 4096 x 256 (+ ``extra``) entries drawn with replacement from the N_SLAB rows,
    three small zones and an empty one: 4096 slots -> S = 128; one entry more -> S = 64."""
    gen = torch.Generator().manual_seed(41)
    big = torch.randint(0, N_SLAB, (BIG + 1,), generator=gen)[:BIG + extra]     # the same first BIG entries
    small = [torch.randint(0, N_SLAB, (s,), generator=gen) for s in (1, 17, 200)]
    return Zones.from_lists([big] + small + [[]], N_SLAB)


# (zones, steps per launch, the T of the GPU tests: each runs as two launches or more)
SLAB_SETS = {"default": (default_slab_zones, 1024, (1028, 1027, 1032)),
             "shrunk": (big_zones, 128, (132, 131, 260)),
             "floor": (lambda: big_zones(1), 64, (68,))}


def steps_per_launch(zones):
    """S, recovered from the launch query (the ABI does not report it): the units of a launch,
    chunks x tiles of 64 steps, grow with every further tile up to S steps and not beyond, and
    with them ``grid`` (few chunks) or ``iters`` (4096 chunks or more)."""
    for t in range(64, 4096, 64):
        if zones.launch(t + 1) == zones.launch(t):
            return t
        assert zones.launch(t + 64) != zones.launch(t)
    raise AssertionError("the launch keeps growing")
