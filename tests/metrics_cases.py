"""The rollout-metrics kernel (msw_rollout_metrics, csrc/metrics.hip) as test cases: planted-value
inputs, a float64 restatement of its sums and counts and of what ``rollout_metrics`` composes from
them, and wrong variants ("mutants") of that restatement, each a plausible kernel error.

A plain module (no test in it), shared by tests/test_metrics.py (CPU: the restatement against
oracle/metrics_ref.py, every mutant caught by a named case) and tests/test_gpu_metrics.py (the
kernel against the restatement).  numpy only.

Grid data (``make_pair``): depths on a 2^-12 grid in [0, 2], discharges on the same grid in
[-2, 2], areas on a 2^-4 grid in [1, 64].  Then ph - rh is exact in fp32, every term of the ten
sums is a multiple of 2^-24 (2^-16 for area * h) below 2^7, and a sum over fewer than 2^22 rows
stays below 2^53 of those units: each sum is exact in fp64 in ANY order of additions, so the kernel
must equal the restatement bit for bit.  Full-precision data (``make_pair_full``): the terms are
still exact in fp64 (a product of two floats), only the order of n additions differs, and two
orders are each within (n - 1) 2^-53 sum|term| of the true sum: ``bound`` is 2 n 2^-53 sum|term|.
"""
import numpy as np

THR4 = (0.0, 0.0625, 0.25, 1.0)   # on the depth grid: equality with a threshold really occurs
STEP = 2.0 ** -12
KINDS = 12                        # planted row kinds, cycling over the row index
ROWS_PER_WG, MAX_WGS, T_CHUNK = 256, 512, 32   # csrc/metrics.hip: kThreads, kMaxParts, kTChunk
ROUND = ROWS_PER_WG * MAX_WGS     # rows of one full round of the grid-stride row loop
N_SUMS = 10


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def make_pair(n, T, seed, thr=THR4, area=False, full=False):
    """-> pred, real [n, 2, T] float32 (and area [n] float32 with area=True).  Row i is of kind
    i % 12:
      0  pred == real in both variables (outside mask_on_water)
      1  only dh != 0            2  only dv != 0
      3  dh = 0 through 0 - (-0.0), dv = 0 (outside the mask; -0.0 is not above threshold 0)
      4  pred depth exactly at thr[t % 4]      5  real depth there      6  both
      7  pred one step above thr[t % 4], real one step below (never below 0)
      8  always dry (both depths 0)            9  always wet (both depths > 1)
      10, 11  plain random
    About 45 % of the random depths and 30 % of the random discharges are exactly 0, so pairs
    with dh = dv = 0 also occur by chance.  full=False: values on the 2^-12 grid; full=True: any
    fp32 value of the same ranges, the steps of kind 7 one ulp."""
    rng = np.random.default_rng(7_000_000 + seed)
    thr4 = np.array(list(thr) + list(THR4)[len(thr):], np.float32)[:4]

    def depth():
        u = rng.random((n, T))
        h = u * 2 if full else np.round(u * 2 * 4096) / 4096
        return _f32(np.where(rng.random((n, T)) < 0.45, 0.0, h))

    def discharge():
        u = rng.random((n, T)) * 4 - 2
        q = u if full else np.round(u * 4096) / 4096
        return _f32(np.where(rng.random((n, T)) < 0.3, 0.0, q))

    ph, rh, pq, rq = depth(), depth(), discharge(), discharge()
    one = np.float32(STEP)
    up = (lambda v: np.nextafter(v, np.float32(4))) if full else (lambda v: _f32(v + one))
    down = (lambda v: np.nextafter(v, np.float32(-4))) if full else (lambda v: _f32(v - one))
    kind = np.arange(n) % KINDS
    at = thr4[np.arange(T) % 4][None, :]
    k = kind == 0
    ph[k], pq[k] = rh[k], rq[k]
    k = kind == 1
    pq[k] = rq[k]
    ph[k] = np.where(ph[k] == rh[k], np.where(rh[k] < 1, up(rh[k]), down(rh[k])), ph[k])
    k = kind == 2
    ph[k] = rh[k]
    pq[k] = np.where(pq[k] == rq[k], np.where(rq[k] < 1, up(rq[k]), down(rq[k])), pq[k])
    k = kind == 3
    ph[k], rh[k], pq[k] = 0.0, -0.0, rq[k]
    ph[kind == 4] = at
    rh[kind == 5] = at
    ph[kind == 6] = at
    rh[kind == 6] = at
    ph[kind == 7] = up(at)
    rh[kind == 7] = np.maximum(down(at), np.float32(0))
    k = kind == 8
    ph[k], rh[k] = 0.0, 0.0
    k = kind == 9
    ph[k] = np.clip(ph[k], 1 + 2 * STEP, 2)
    rh[k] = np.clip(rh[k], 1 + 2 * STEP, 2)
    pred, real = _f32(np.stack((ph, pq), 1)), _f32(np.stack((rh, rq), 1))
    if not area:
        return pred, real
    u = rng.random(n) * 63 + 1
    return pred, real, _f32(u if full else np.round(u * 16) / 16)


def make_pair_full(n, T, seed, thr=THR4, area=False):
    """``make_pair`` with full-precision fp32 values: compared within ``bound``."""
    return make_pair(n, T, seed, thr, area, full=True)


def _reference(pred, real, ranges, thr, area=None, mutant=None, round_rows=ROUND, abs_terms=False):
    pred, real = np.asarray(pred, np.float32), np.asarray(real, np.float32)
    S, T, K = len(ranges), pred.shape[2], len(thr)
    sums = np.zeros((S, T, N_SUMS))
    counts = np.zeros((S, T, K, 4), np.int64)
    for g, (s, e) in enumerate(ranges):
        n = e - s
        if mutant == "tail_rows_dropped":
            n = n // ROWS_PER_WG * ROWS_PER_WG
        if mutant == "later_row_iterations_dropped":
            n = min(n, round_rows)
        if n == 0:
            continue
        lo = 0 if mutant == "row0_ignored" else s
        p, r = pred[lo:lo + n], real[lo:lo + n]
        ph, rh = p[:, 0, :], r[:, 0, :]
        dh, dv = ph - rh, p[:, 1, :] - r[:, 1, :]          # the fp32 difference comes first
        ah, av = np.abs(dh.astype(np.float64)), np.abs(dv.astype(np.float64))
        if mutant == "squares_in_fp32":
            qh, qv = (dh * dh).astype(np.float64), (dv * dv).astype(np.float64)
        else:
            qh, qv = ah * ah, av * av
        if mutant == "mask_and":
            wet = (dh != 0) & (dv != 0)
        else:
            wet = (dh != 0) | (dv != 0)
        out = sums[g]
        for i, term in enumerate((ah, av, qh, qv)):
            out[:, i] = term.sum(0)
            out[:, 4 + i] = np.where(wet, term, 0.0).sum(0)
        out[:, 8] = wet.sum(0)
        if area is not None:
            a_lo = 0 if mutant == "area_by_local_row" else lo
            a = np.asarray(area, np.float32)[a_lo:a_lo + n].astype(np.float64)[:, None]
            h64 = ph.astype(np.float64)
            out[:, 9] = (a * (np.abs(h64) if abs_terms else h64)).sum(0)
        for k, t in enumerate(thr):
            t = np.float32(t)
            P, R = (ph >= t, rh >= t) if mutant == "ge_for_gt" else (ph > t, rh > t)
            tp, tn, fp, fn = (P & R).sum(0), (~P & ~R).sum(0), (P & ~R).sum(0), (~P & R).sum(0)
            if mutant == "fp_fn_swapped":
                fp, fn = fn, fp
            counts[g, :, k, :] = np.stack((tp, tn, fp, fn), -1)
    sums += 0.0   # -0.0 -> +0.0: the kernel's accumulators start from +0.0
    if mutant == "steps_from_32_dropped":
        sums[:, T_CHUNK:], counts[:, T_CHUNK:] = 0.0, 0
    if mutant == "ragged_time_chunk_dropped" and T % T_CHUNK:
        sums[:, T // T_CHUNK * T_CHUNK:], counts[:, T // T_CHUNK * T_CHUNK:] = 0.0, 0
    if mutant == "sums_leak_into_next_simulation":
        clean = sums.copy()
        for g in range(1, S):
            if ranges[g][1] > ranges[g][0]:
                sums[g] += clean[g - 1]
    return sums, counts


def reference(pred, real, ranges, thr, area=None):
    """The ten sums [S, T, 10] (float64) and the confusion counts [S, T, n_thr, 4] (int64: TP, TN,
    FP, FN) of include/mswegnn.h msw_rollout_metrics, per simulation (rows ranges[g][0] ..
    ranges[g][1] - 1) and step, in plain numpy float64.  An empty simulation gives zeros."""
    return _reference(pred, real, ranges, thr, area)


def bound(pred, real, ranges, area=None):
    """[S, T, 10]: 2 n 2^-53 sum|term|, the distance two summation orders of n exact terms can be
    apart (0 for the row count, which is exact)."""
    mag = _reference(pred, real, ranges, (), area, abs_terms=True)[0]
    n = np.array([e - s for s, e in ranges], np.float64)[:, None, None]
    b = 2 * n * 2.0 ** -53 * mag
    b[..., 8] = 0.0
    return b


def _mutant(name):
    def f(pred, real, ranges, thr, area=None, round_rows=ROUND):
        return _reference(pred, real, ranges, thr, area, mutant=name, round_rows=round_rows)
    f.__name__ = name
    return f


# Wrong variants of ``reference``: what the kernel would compute with one plausible error.
mutants = {name: _mutant(name) for name in (
    "tail_rows_dropped",               # nrows rounded down to a multiple of 256
    "later_row_iterations_dropped",    # only the first round of the grid-stride row loop
    "steps_from_32_dropped",           # only the first time chunk
    "ragged_time_chunk_dropped",       # a last time chunk of fewer than 32 steps
    "ge_for_gt",                       # flooded iff h >= thr
    "fp_fn_swapped",
    "mask_and",                        # mask_on_water as dh != 0 && dv != 0
    "row0_ignored",                    # rows 0 .. nrows - 1 whatever the range
    "area_by_local_row",               # area[i] for area[row0 + i]
    "sums_leak_into_next_simulation",  # the shared scratch not overwritten between simulations
    "squares_in_fp32",                 # (double)(dh * dh) for (double)dh * dh
)}


def compose(sums, counts, ranges, thr, mass=None, pred=None):
    """What ``mswegnn.metrics.rollout_metrics`` returns, from the sums and counts, in float64:
    rmse, mae [S, 2]; rmse_water, mae_water [S, 2]; csi, f1 {thr: [S, T]}; with ``mass`` (the
    wrapper's dict: node_bc in graph rows) and ``pred`` also mass_loss [S, T - 1]."""
    sums, counts = np.asarray(sums, np.float64), np.asarray(counts)
    S, T = sums.shape[:2]
    n0 = np.array([e - s for s, e in ranges], np.float64)[:, None, None]
    out = {}
    with np.errstate(all="ignore"):
        out["mae"] = (sums[..., 0:2] / n0).mean(1)
        out["rmse"] = np.sqrt(sums[..., 2:4] / n0).mean(1)
        cnt = sums[..., 8].sum(1)[:, None]
        out["mae_water"] = sums[..., 4:6].sum(1) / cnt
        out["rmse_water"] = np.sqrt(sums[..., 6:8].sum(1) / cnt)
        out["csi"], out["f1"] = {}, {}
        for k, t in enumerate(thr):
            tp, tn, fp, fn = (counts[:, :, k, i].astype(np.float64) for i in range(4))
            out["csi"][float(t)] = tp / (tp + fn + fp)
            out["f1"][float(t)] = tp / (tp + 0.5 * (fn + fp))
    if mass is not None:
        area = np.asarray(mass["area"], np.float64)
        per = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * S   # noqa: E731
        tres, lens = per(mass.get("temporal_res", 1)), per(mass["edge_bc_length"])
        res = np.zeros((S, max(T - 1, 0)))
        for g in range(S):
            rows = np.asarray(mass["node_bc"][g]).reshape(-1).astype(np.int64)
            h = np.asarray(pred, np.float32)[rows, 0, :].astype(np.float64)
            corr = (area[rows][:, None] * (h[:, 1:] - h[:, :-1])).sum(0)
            bc = np.atleast_2d(np.asarray(mass["bc"][g], np.float64))
            q = 0.5 * (bc[:, 1:T] + bc[:, 2:T + 1])
            inflow = (q * np.asarray(lens[g], np.float64).reshape(-1, 1)).sum(0) * (60.0 * float(np.asarray(tres[g])))
            res[g] = (sums[g, 1:, 9] - sums[g, :-1, 9] - inflow - corr) / 1e6
        out["mass_loss"] = res
    return out


def same_bits(a, b):
    """float64 arrays equal bit for bit, NaN matching NaN."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and \
        np.array_equal(a.view(np.int64)[~nan], b.view(np.int64)[~nan])


def differs(got, want):
    """A mutant's (sums, counts) differ from the restatement's in an asserted value."""
    return not (same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]))


def rows_for_iterations(launch, rounds):
    """A row count that takes exactly ``rounds`` rounds of the row loop, the last one ragged
    (a third of the grid and 13 rows), from the launch query ``launch(nrows, T) -> (grid,
    time_chunks, rows_per_wg, iters)`` asked at a huge row count."""
    grid, _, per_wg, _ = launch(1 << 40, 3)
    return grid * per_wg * (rounds - 1) + per_wg * (grid // 3) + 13


def layout(sizes, gaps):
    """Row ranges of consecutive simulations of ``sizes`` rows, ``gaps[g]`` rows (coarse scales,
    in a real batch) before simulation g -> (ranges, total rows with a trailing gap of 3)."""
    ranges, at = [], 0
    for n, gap in zip(sizes, gaps):
        at += gap
        ranges.append((at, at + n))
        at += n
    return ranges, at + 3


def poison(arrays, ranges, value):
    """Copies of the [N, ...] arrays with every row outside the ranges set to ``value``."""
    inside = np.zeros(arrays[0].shape[0], bool)
    for s, e in ranges:
        inside[s:e] = True
    out = []
    for a in arrays:
        a = a.copy()
        a[~inside] = value
        out.append(a)
    return out


# Named cases, run by the GPU suite (test_named_cases) and by the CPU mutant test, which lists for
# every mutant the cases that catch it.  sizes / gaps -> ``layout``; "iters": the row count comes
# from the launch query (``rows_for_iterations``).
CASES = {
    "one_row": dict(sizes=[1], gaps=[0], T=1, n_thr=1, area=True, seed=1),
    "tail_257": dict(sizes=[257], gaps=[0], T=3, n_thr=4, area=True, seed=2),
    "full_block_256": dict(sizes=[256], gaps=[0], T=3, n_thr=2, area=False, seed=3),
    "row0_5": dict(sizes=[255], gaps=[5], T=31, n_thr=1, area=True, seed=4),
    "T33": dict(sizes=[65], gaps=[0], T=33, n_thr=2, area=False, seed=5),
    "T64": dict(sizes=[63], gaps=[5], T=64, n_thr=0, area=True, seed=6),
    "T65": dict(sizes=[64], gaps=[5], T=65, n_thr=4, area=False, seed=7),
    "two_iterations": dict(iters=2, gaps=[0], T=3, n_thr=2, area=True, seed=8),
    "three_iterations": dict(iters=3, gaps=[0], T=3, n_thr=2, area=True, seed=9),
    "five_sims": dict(sizes=[300, 0, 1499, 17, 257], gaps=[4, 9, 0, 131, 1], T=5, n_thr=3, area=True, seed=10),
    "full_1499": dict(sizes=[1499], gaps=[5], T=33, n_thr=4, area=True, seed=11, full=True),
}

# mutant -> the named cases that must catch it (tests/test_metrics.py asserts each, and that
# no mutant is caught by none)
KILLED_BY = {
    "tail_rows_dropped": ["one_row", "tail_257"],
    "later_row_iterations_dropped": ["two_iterations", "three_iterations"],
    "steps_from_32_dropped": ["T33", "T64", "T65"],
    "ragged_time_chunk_dropped": ["T33", "T65", "one_row"],
    "ge_for_gt": ["tail_257", "T65"],
    "fp_fn_swapped": ["tail_257", "full_1499"],
    "mask_and": ["tail_257", "full_block_256"],
    "row0_ignored": ["row0_5", "T64", "five_sims"],
    "area_by_local_row": ["row0_5", "T64", "five_sims"],
    "sums_leak_into_next_simulation": ["five_sims"],
    "squares_in_fp32": ["full_1499"],   # only asked of the full-precision data
}


def build_case(spec, launch):
    """-> dict(pred, real, area or None, ranges, thr, T, full) of a CASES entry."""
    sizes = spec.get("sizes") or [rows_for_iterations(launch, spec["iters"])]
    ranges, total = layout(sizes, spec["gaps"])
    thr = THR4[:spec["n_thr"]]
    full = spec.get("full", False)
    data = make_pair(total, spec["T"], spec["seed"], thr, area=True, full=full)
    return dict(pred=data[0], real=data[1], area=data[2] if spec["area"] else None, ranges=ranges, thr=thr,
                T=spec["T"], full=full)
