"""The ensemble kernels (msw_ensemble_steps_update, msw_ensemble_maps, csrc/ensemble.hip) as test
cases: planted-value inputs, a numpy restatement of both kernels that shares nothing with the
module's torch one, and wrong variants ("mutants") of that restatement, each a plausible kernel
error.

A plain module (no test in it), shared by tests/test_ensemble.py (CPU: the module's torch path
against the restatement, every mutant caught by a named case) and tests/test_gpu_ensemble.py (the
kernels against the restatement).  numpy only.

The restatement: the mean is a sequential float64 loop over the members in list order, divided by
M and rounded to float32; order statistics are ``np.argsort(kind="stable")`` along the members,
steps under the key ``where(s < 0, INT32_MAX, s)``; ``check_inverted_cdf`` ties the ranks to
``np.quantile(method="inverted_cdf")``.

Data (``make_members``): depths on a 2^-12 grid in [0, 1.5], 45 % of them exactly 0, so that ties
across members are the normal case; cell i is of kind i % 10:
  0  all members equal                      1  all members dry (0)
  2  never above the smallest positive threshold (never wet there: every first_wet is -1)
  3  exactly one member wet (member (i // 10) % M above every threshold, the others 0)
  4  depths exactly at thr[(t + m) % 4]     5  one grid step above it (even m) / below it (odd m)
  6  all members > 0 (a minimum seeded with 0 would stay 0)
  7, 8, 9  plain random
The members lie in shuffled order in an [N, 2, T] array with gaps between and around them whose
depths are NaN or 7e8; every discharge is NaN: the kernel never reads that half.
"""
import numpy as np

THR4 = (0.0625, 0.25, 0.0, 1.0)   # on the depth grid: equality with a threshold really occurs
STEP = 2.0 ** -12
KINDS = 10
INT32_MAX = np.iinfo(np.int32).max
CANARY_F, CANARY_I = np.float32(-12345.5), np.int32(-123456789)
STEP_NAMES = ("wet_members", "h_mean", "h_min", "h_max")
MAP_NAMES = ("exceed_members", "mean", "rank_values", "members_with_step", "rank_steps")


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def make_members(n, M, T, seed, full=False):
    """-> h [M, n, T] float32, the depths of every member (see the module docstring)."""
    rng = np.random.default_rng(9_000_000 + seed)
    u = rng.random((M, n, T)) * 1.5
    h = _f32(u if full else np.round(u * 4096) / 4096)
    h = np.where(rng.random((M, n, T)) < 0.45, np.float32(0), h)
    thr = np.array(THR4, np.float32)
    one = np.float32(STEP)
    kind = np.arange(n) % KINDS
    m_idx, t_idx = np.arange(M)[:, None, None], np.arange(T)[None, None, :]
    k = kind == 0
    h[:, k] = h[:1, k]
    h[:, kind == 1] = 0
    k = kind == 2
    h[:, k] = np.minimum(h[:, k], np.float32(0.0625))
    k = np.nonzero(kind == 3)[0]
    h[:, k] = 0
    h[(k // KINDS) % M, k] = np.float32(1.25) + one * (np.arange(T) % 3)[None, :]
    at = np.broadcast_to(thr[(t_idx + m_idx) % 4], (M, 1, T))
    h[:, kind == 4] = at
    beside = np.where(m_idx % 2 == 0, at + one, np.maximum(at - one, np.float32(0)))
    h[:, kind == 5] = beside
    k = kind == 6
    h[:, k] = np.clip(h[:, k], np.float32(0.5), None)
    return _f32(h)


def place(h, seed):
    """The members of ``h`` [M, n, T] in shuffled order inside a poisoned [N, 2, T] array
    -> (pred, member_row0 [M] int64: the row of cell 0 of member m)."""
    M, n, T = h.shape
    rng = np.random.default_rng(9_500_000 + seed)
    order = rng.permutation(M)
    gaps = rng.integers(1, 6, M + 1)
    N = int(M * n + gaps.sum())
    pred = np.full((N, 2, T), np.nan, np.float32)
    row0 = np.zeros(M, np.int64)
    at = 0
    for slot, m in enumerate(order):
        pred[at:at + gaps[slot], 0] = np.nan if slot % 2 else np.float32(7e8)
        at += int(gaps[slot])
        row0[m] = at
        pred[at:at + n, 0] = h[m]
        at += n
    pred[at:, 0] = np.float32(7e8)
    return pred, row0


def gather(pred, row0, n):
    """[M, n, T]: the depths of the members at ``row0``."""
    return np.stack([np.asarray(pred, np.float32)[r:r + n, 0, :] for r in row0])


# ------------------------------------------------------------------ kernel A
def steps_reference(pred, row0, n, thr, t_begin=0, t_count=None, T_out=None, t_out0=0, mutant=None):
    """msw_ensemble_steps_update in numpy -> {name: array [.., n, T_out]}, the window's columns
    filled and every other column holding the canary."""
    T = pred.shape[2]
    t_count = T - t_begin if t_count is None else t_count
    T_out = t_count if T_out is None else T_out
    rows = list(row0)
    M = len(rows)
    if mutant == "row0_ignored":
        rows = [m * n for m in range(M)]
    tb = 0 if mutant == "t_begin_ignored" else t_begin
    h = gather(pred, rows, n)[:, :, tb:tb + t_count]
    used = h[:-1] if mutant == "last_member_dropped" and M > 1 else h
    if mutant == "mean_fp32":
        s = np.zeros(h.shape[1:], np.float32)
        for m in range(used.shape[0]):
            s = s + used[m]
        s = s.astype(np.float64)
    else:
        s = np.zeros(h.shape[1:], np.float64)
        for m in range(used.shape[0]):          # sequential, member order
            s = s + used[m].astype(np.float64)
    res = {"h_mean": (s / np.float64(M)).astype(np.float32)}
    res["h_min"] = np.minimum(used.min(0), np.float32(0)) if mutant == "min_seeded_0" else used.min(0)
    res["h_max"] = used.max(0)
    cmp = np.greater_equal if mutant == "ge_for_gt" else np.greater
    res["wet_members"] = np.stack([cmp(used, np.float32(t)).sum(0).astype(np.int32) for t in thr]) if len(thr) \
        else np.zeros((0,) + h.shape[1:], np.int32)
    col0 = 0 if mutant == "t_out0_ignored" else t_out0
    out = {}
    for k, v in res.items():
        full = np.full(v.shape[:-1] + (T_out,), CANARY_I if v.dtype == np.int32 else CANARY_F, v.dtype)
        full[..., col0:col0 + t_count] = v
        out[k] = full
    return out


# ------------------------------------------------------------------ kernel B
def member_maps(h, thr):
    """Per-member maps of depths ``h`` [M, n, T]: values = max over time [M, n] float32 and, per
    threshold, steps = the first t with h > thr, else -1 [n_thr, M, n] int32."""
    values = h.max(2)
    steps = []
    for t in thr:
        wet = h > np.float32(t)
        steps.append(np.where(wet.any(2), wet.argmax(2), -1).astype(np.int32))
    return _f32(values), np.stack(steps) if steps else np.zeros((0,) + values.shape, np.int32)


def maps_reference(values, steps, thr, ranks, mutant=None):
    """msw_ensemble_maps in numpy -> the outputs of msw_ensemble_maps_out (those of a None input
    are missing)."""
    out = {}
    ranks = np.asarray(ranks, np.int64).reshape(-1)
    src = values if values is not None else steps
    M = src.shape[0]
    if mutant == "rank_plus_one":
        ranks = np.minimum(ranks + 1, M - 1)
    if mutant == "rank_minus_one":
        ranks = np.maximum(ranks - 1, 0)
    cols = np.arange(src.shape[1])[None, :]
    if values is not None:
        v = np.asarray(values, np.float32)
        used = v[:-1] if mutant == "last_member_dropped" and M > 1 else v
        cmp = np.greater_equal if mutant == "ge_for_gt" else np.greater
        out["exceed_members"] = np.stack([cmp(used, np.float32(t)).sum(0).astype(np.int32) for t in thr]) \
            if len(thr) else np.zeros((0, v.shape[1]), np.int32)
        if mutant == "mean_fp32":
            s = np.zeros(v.shape[1], np.float32)
            for m in range(used.shape[0]):
                s = s + used[m]
            s = s.astype(np.float64)
        else:
            s = np.zeros(v.shape[1], np.float64)
            for m in range(used.shape[0]):
                s = s + used[m].astype(np.float64)
        out["mean"] = (s / np.float64(M)).astype(np.float32)
        order = np.argsort(used, axis=0, kind="stable")
        out["rank_values"] = used[order[np.minimum(ranks, used.shape[0] - 1)], cols]
    if steps is not None:
        s = np.asarray(steps, np.int32)
        used = s[:-1] if mutant == "last_member_dropped" and M > 1 else s
        out["members_with_step"] = (used >= 0).sum(0).astype(np.int32)
        key = used if mutant == "minus1_first" else np.where(used < 0, INT32_MAX, used)
        order = np.argsort(key, axis=0, kind="stable")
        out["rank_steps"] = used[order[np.minimum(ranks, used.shape[0] - 1)], cols]
    return out


def check_inverted_cdf(values, probs, ranks):
    """The restatement's value of rank ``ranks[j]`` is numpy's inverted_cdf ``probs[j]``-quantile
    along the members."""
    got = maps_reference(values, None, (), ranks)["rank_values"]
    for j, p in enumerate(probs):
        want = np.quantile(np.asarray(values, np.float64), p, axis=0, method="inverted_cdf").astype(np.float32)
        assert np.array_equal(got[j], want), p


def _mutant(fn, name):
    def f(*a, **kw):
        return fn(*a, mutant=name, **kw)
    f.__name__ = name
    return f


STEP_MUTANTS = ("ge_for_gt", "last_member_dropped", "row0_ignored", "mean_fp32", "min_seeded_0", "t_begin_ignored",
                "t_out0_ignored")
MAP_MUTANTS = ("ge_for_gt", "last_member_dropped", "minus1_first", "rank_plus_one", "rank_minus_one", "mean_fp32")
step_mutants = {k: _mutant(steps_reference, k) for k in STEP_MUTANTS}
map_mutants = {k: _mutant(maps_reference, k) for k in MAP_MUTANTS}


def same(a, b):
    """Two result dicts hold the same arrays, bit for bit (-0.0 == 0.0 aside)."""
    return a.keys() == b.keys() and all(a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]) for k in a)


# Named cases: n cells, M members, T steps; window (t_begin, t_count) into columns t_out0 .. of
# T_out; ranks for the maps.  Run by the GPU suite and by the CPU mutant test.
CASES = {
    "m1": dict(n=1, M=1, T=1, n_thr=1, seed=1, ranks=(0,)),
    "m3": dict(n=65, M=3, T=5, n_thr=4, seed=2, ranks=(0, 1, 2)),
    "m64": dict(n=63, M=64, T=3, n_thr=2, seed=3, ranks=(0, 6, 31, 32, 57, 63, 0, 0)),
    "window": dict(n=64, M=2, T=47, n_thr=2, seed=4, t_begin=5, t_count=17, T_out=30, t_out0=7, ranks=(0, 1)),
    "full_m7": dict(n=257, M=7, T=48, n_thr=4, seed=5, full=True, ranks=(0, 3, 6)),
}

# mutant -> the named cases that must catch it (tests/test_ensemble.py asserts each)
STEPS_KILLED_BY = {
    "ge_for_gt": ["m3", "m64"],
    "last_member_dropped": ["m3", "m64"],
    "row0_ignored": ["m3", "m64", "window"],
    "mean_fp32": ["full_m7"],             # only asked of the full-precision data
    "min_seeded_0": ["m3", "m64"],
    "t_begin_ignored": ["window"],
    "t_out0_ignored": ["window"],
}
MAPS_KILLED_BY = {
    "ge_for_gt": ["m3", "m64"],
    "last_member_dropped": ["m3", "m64"],
    "minus1_first": ["m3", "m64"],
    "rank_plus_one": ["m3", "m64"],
    "rank_minus_one": ["m3", "m64"],
    "mean_fp32": ["full_m7"],
}


def build_case(spec):
    """-> dict(pred [N, 2, T], row0, h [M, n, T], n, M, T, thr, window keywords, ranks, values
    [M, n], steps [n_thr, M, n]) of a CASES entry."""
    n, M, T = spec["n"], spec["M"], spec["T"]
    thr = THR4[:spec["n_thr"]]
    h = make_members(n, M, T, spec["seed"], spec.get("full", False))
    pred, row0 = place(h, spec["seed"])
    values, steps = member_maps(h, thr)
    window = dict(t_begin=spec.get("t_begin", 0), t_count=spec.get("t_count", T), T_out=spec.get("T_out", T),
                  t_out0=spec.get("t_out0", 0))
    return dict(pred=pred, row0=row0, h=h, n=n, M=M, T=T, thr=thr, window=window, ranks=spec["ranks"],
                values=values, steps=steps)


def cells_for_rounds(launch, M, T, rounds):
    """A cell count that takes exactly ``rounds`` rounds of kernel A's cell loop, the last one
    ragged (a third of the grid and 13 cells), from the launch query ``launch(n, M, t_count) ->
    (grid, cells_per_wg, iters)`` asked at a huge cell count."""
    grid, per_wg, _ = launch(1 << 40, M, T)
    return grid * per_wg * (rounds - 1) + per_wg * (grid // 3) + 13


def check_products(out, pred, ranges, thr, probs, ranks, to_np=np.asarray):
    """The products of ``mswegnn.ensemble.rollout_ensemble`` (``out``) equal the restatement
    applied to the kept rollout ``pred`` [N, 2, T] (numpy); ``to_np`` brings a product to numpy."""
    row0, n = [s for s, _ in ranges], ranges[0][1] - ranges[0][0]
    want = steps_reference(pred, row0, n, thr)
    st = out["steps"]
    for k in ("h_mean", "h_min", "h_max"):
        assert np.array_equal(to_np(st[k]), want[k]), k
    for i, t in enumerate(thr):
        assert np.array_equal(to_np(st["wet_members"][t]), want["wet_members"][i]), t
    values, steps = member_maps(gather(pred, row0, n), thr)
    mp = out["maps"]
    w = maps_reference(values, None, thr, ranks)
    assert np.array_equal(to_np(mp["h_max"]["mean"]), w["mean"])
    for i, t in enumerate(thr):
        assert np.array_equal(to_np(mp["h_max"]["exceed_members"][t]), w["exceed_members"][i]), t
    for j, p in enumerate(probs):
        assert np.array_equal(to_np(mp["h_max"]["quantiles"][p]), w["rank_values"][j]), p
    for i, t in enumerate(thr):
        w = maps_reference(None, steps[i], (), ranks)
        assert np.array_equal(to_np(mp["first_wet"][t]["members_with_step"]), w["members_with_step"]), t
        for j, p in enumerate(probs):
            assert np.array_equal(to_np(mp["first_wet"][t]["step_quantiles"][p]), w["rank_steps"][j]), (t, p)
