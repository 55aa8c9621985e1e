"""The ensemble-scores kernel (msw_ensemble_scores_update, csrc/scores.hip) as test cases:
planted-value members and truths, a numpy restatement that shares nothing with the module's torch
path or with the sorted formula, and wrong variants ("mutants") of that restatement, each a
plausible kernel error.

A plain module (no test in it), shared by tests/test_scores.py (CPU) and tests/test_gpu_scores.py.
numpy only.  The reference has no ensemble code: this restatement is the yardstick.

The restatement.  Per cell and step, in float64 on the converted float32 depths: a = sum_m
|h_m - y| and b = sum_{m<m'} |h_m - h_m'| by explicit loops over the members and the pairs, S and
sum h^2 by a loop in member order, e = S - M y, v = M sum h^2 - S^2; a NaN depth makes the five
terms NaN.  sums = the terms added over the cells; the table by comparisons and counting;
cell_crps = the carried value plus M a - b, step after step.

Data.  Members: ``ensemble_cases.make_members`` (2^-12 grid in [0, 1.5], 45 % zeros, kinds by cell).
Truth (``make_truth``), cell i of kind (i // 2) % 7 -- so that the truth's kinds meet the members'
kinds (i % 10) in every combination:
  0  equal to member 0                  1  dry
  2  exactly at THR4[t % 4]             3  one grid step beside it (above at even t, below at odd t)
  4  above every member                 5  below every positive member (dry where there is none)
  6  random on the grid (``full``: any float32)
On grid data every term is a multiple of 2^-24 and every sum stays below 2^53 such units
(``build_case`` asserts both): every float64 sum is exact, in any order, and everything is
compared bit for bit.
"""
import numpy as np

import ensemble_cases as ec

THR4, STEP = ec.THR4, ec.STEP
TRUTH_KINDS = 7
SUM_NAMES = ("a", "b", "abs_e", "e2", "v")
NAMES = ("sums", "reliability", "cell_crps")
CANARY_D, CANARY_L = np.float64(-12345.5), np.int64(-123456789)
UNIT = 2.0 ** -24


def make_truth(h, seed, full=False):
    """-> y [n, T] float32, the truth depths for the members ``h`` [M, n, T]."""
    M, n, T = h.shape
    rng = np.random.default_rng(8_000_000 + seed)
    u = rng.random((n, T)) * 1.5
    y = ec._f32(u if full else np.round(u * 4096) / 4096)
    y = np.where(rng.random((n, T)) < 0.3, np.float32(0), y)
    kind = (np.arange(n) // 2) % TRUTH_KINDS
    thr = np.array(THR4, np.float32)
    one = np.float32(STEP)
    t_idx = np.arange(T)
    y[kind == 0] = h[0, kind == 0]
    y[kind == 1] = 0
    at = np.broadcast_to(thr[t_idx % 4], (n, T))
    y[kind == 2] = at[kind == 2]
    beside = np.where(t_idx % 2 == 0, at + one, np.maximum(at - one, np.float32(0)))
    y[kind == 3] = beside[kind == 3]
    y[kind == 4] = (h.max(0) + np.float32(0.5))[kind == 4]
    pos = np.where(h > 0, h, np.float32(np.inf)).min(0)
    below = np.where(np.isfinite(pos), np.maximum(pos - one, np.float32(0)), np.float32(0))
    y[kind == 5] = below[kind == 5]
    return ec._f32(y)


def place_truth(y, seed, T_truth=None, t_truth0=0):
    """The truth ``y`` [n, T] in columns ``t_truth0 ..`` of rows ``truth_row0 ..`` of its own
    poisoned [n + gaps, 2, T_truth] array (NaN / 7e8 around it, every discharge NaN)
    -> (truth, truth_row0)."""
    n, T = y.shape
    T_truth = T + t_truth0 if T_truth is None else T_truth
    rng = np.random.default_rng(8_500_000 + seed)
    before, after = (int(v) for v in rng.integers(1, 6, 2))
    truth = np.full((n + before + after, 2, T_truth), np.nan, np.float32)
    truth[:before, 0] = np.float32(7e8)
    truth[before:before + n, 0] = np.float32(7e8) if seed % 2 else np.nan
    truth[before:before + n, 0, t_truth0:t_truth0 + T] = y
    return truth, before


# ------------------------------------------------------------------ the restatement
def terms(h, y, mutant=None):
    """The five terms per cell and step, float64 [5, n, t], of members ``h`` [M, n, t] and truth
    ``y`` [n, t] (float32), by explicit loops over the members and over the pairs m < m'."""
    M = h.shape[0]
    hd, yd = h.astype(np.float64), y.astype(np.float64)
    used = range(M - 1) if mutant == "last_member_dropped" and M > 1 else range(M)
    a, b = np.zeros_like(yd), np.zeros_like(yd)
    S, Q = np.zeros_like(yd), np.zeros_like(yd)
    for m in used:
        a = a + np.abs(hd[m] - yd)
        S = S + hd[m]
        Q = Q + hd[m] * hd[m]
        for m2 in used:
            if m2 > m or (mutant == "pairs_twice" and m2 != m):
                b = b + np.abs(hd[m] - hd[m2])
    if mutant == "rank_counts_itself":   # m <= m' adds only zeros to the pair form; in the rank form it is + 2 S
        b = b + 2 * S
    Mf = np.float64(M)
    e = S - Mf * yd
    v = Q - S * S if mutant == "v_unscaled" else Mf * Q - S * S
    e2 = (e.astype(np.float32) * e.astype(np.float32)).astype(np.float64) if mutant == "e2_fp32" else e * e
    bad = np.isnan(a)
    b, v = np.where(bad, a, b), np.where(bad, a, v)
    return np.stack([a, b, np.abs(e), e2, v])


def scores_reference(pred, row0, n, truth, truth_row0, t_truth0, thr, t_begin=0, t_count=None, T_out=None, t_out0=0,
                     carried=None, mutant=None):
    """msw_ensemble_scores_update in numpy -> ``sums`` [T_out, 5] float64 and ``reliability``
    [T_out, n_thr, M + 1, 2] int64, the window's columns filled and every other column holding the
    canary, and ``cell_crps`` [n] float64 = ``carried`` (default zeros) plus the window's steps."""
    T = pred.shape[2]
    t_count = T - t_begin if t_count is None else t_count
    T_out = t_count if T_out is None else T_out
    M = len(row0)
    tb = 0 if mutant == "t_begin_ignored" else t_begin
    tr0 = 0 if mutant == "truth_row0_ignored" else truth_row0
    tt0 = 0 if mutant == "t_truth0_ignored" else t_truth0
    h = ec.gather(pred, row0, n)[:, :, tb:tb + t_count]
    y = np.asarray(truth, np.float32)[tr0:tr0 + n, 0, tt0:tt0 + t_count]
    keep = np.ones(n, bool)
    if mutant == "tail_dropped":
        keep = np.arange(n) < n // 64 * 64
    if mutant == "later_rounds_dropped":   # only the first round of a block of 16 cells
        keep = np.arange(n) % 16 < max(64 // max(t_count, 1), 1)
    tm = terms(h, y, mutant)
    sums = np.stack([tm[j][keep].sum(0) if keep.any() else np.zeros(t_count) for j in range(5)], 1)   # [t, 5]
    if mutant == "e2_fp32":
        sums[:, 3] = tm[3][keep].astype(np.float32).sum(0, dtype=np.float32)
    if mutant == "sums_leak":
        sums = np.cumsum(sums, 0)
    used = h[:-1] if mutant == "last_member_dropped" and M > 1 else h
    cmp = np.greater_equal if mutant == "ge_for_gt" else np.greater
    table = np.zeros((t_count, len(thr), M + 1, 2), np.int64)
    for k, th in enumerate(thr):
        th = np.float32(thr[0] if mutant == "table_not_split" else th)
        c = cmp(used, th).sum(0)                                     # [n, t]
        o = cmp(y, th)
        for cc in range(M + 1):
            hit = (c == cc) & keep[:, None]
            table[:, k, cc, 0] = hit.sum(0)
            if mutant == "observed_bin_plus_one":
                if cc + 1 <= M:
                    table[:, k, cc + 1, 1] = (hit & o).sum(0)
            else:
                table[:, k, cc, 1] = (hit & o).sum(0)
    cell = np.zeros(n) if carried is None or mutant == "crps_overwritten" else np.array(carried, np.float64)
    x = np.float64(M) * tm[0] - tm[1]
    for t in range(t_count):                                        # step order, onto the carried value
        cell = cell + np.where(keep, x[:, t], 0.0)
    col0 = t_out0
    out = {"sums": np.full((T_out, 5), CANARY_D, np.float64),
           "reliability": np.full((T_out, len(thr), M + 1, 2), CANARY_L, np.int64), "cell_crps": cell}
    out["sums"][col0:col0 + t_count] = sums
    out["reliability"][col0:col0 + t_count] = table
    return out


def _mutant(name):
    def f(*a, **kw):
        return scores_reference(*a, mutant=name, **kw)
    f.__name__ = name
    return f


MUTANTS = ("pairs_twice", "rank_counts_itself", "ge_for_gt", "truth_row0_ignored", "t_truth0_ignored",
           "t_begin_ignored", "last_member_dropped", "observed_bin_plus_one", "table_not_split", "e2_fp32",
           "v_unscaled", "crps_overwritten", "sums_leak", "tail_dropped", "later_rounds_dropped")
mutants = {k: _mutant(k) for k in MUTANTS}


def same(a, b):
    """Two result dicts hold the same arrays, bit for bit (-0.0 == 0.0 aside; NaN equals NaN)."""
    return a.keys() == b.keys() and all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and
                                        np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f") for k in a)


# Named cases: n cells, M members, T steps; window (t_begin, t_count) into columns t_out0 .. of
# T_out.  ``alias``: the truth is one more range of pred; else it has its own array with T_truth
# columns, the window's first at t_truth0.  ``carried``: cell_crps holds values before the call.
CASES = {
    "m1": dict(n=1, M=1, T=1, n_thr=1, seed=1),
    "m3": dict(n=65, M=3, T=5, n_thr=4, seed=2, alias=True),
    "m64": dict(n=63, M=64, T=3, n_thr=2, seed=3),
    "window": dict(n=64, M=2, T=47, n_thr=2, seed=4, t_begin=5, t_count=17, T_out=30, t_out0=7, T_truth=40,
                   t_truth0=9, carried=True),
    "tail": dict(n=257, M=16, T=8, n_thr=3, seed=6, carried=True),
    "full_m7": dict(n=257, M=7, T=48, n_thr=4, seed=5, full=True),
}
GRID_CASES = tuple(k for k, v in CASES.items() if not v.get("full"))

# mutant -> the named cases that must catch it (tests/test_scores.py asserts each)
KILLED_BY = {
    "pairs_twice": ["m3", "m64", "tail"],
    "rank_counts_itself": ["m3", "m64", "tail"],
    "ge_for_gt": ["m3", "m64", "tail"],
    "truth_row0_ignored": ["m3", "m64", "window", "tail"],
    "t_truth0_ignored": ["window"],
    "t_begin_ignored": ["window"],
    "last_member_dropped": ["m3", "m64", "tail"],
    "observed_bin_plus_one": ["m3", "m64", "tail"],
    "table_not_split": ["m3", "m64", "tail"],
    "e2_fp32": ["m64", "tail"],
    "v_unscaled": ["m3", "m64", "tail"],
    "crps_overwritten": ["window", "tail"],
    "sums_leak": ["m3", "m64", "tail"],
    "tail_dropped": ["m3", "tail"],          # n = 65, 257
    "later_rounds_dropped": ["m3", "window", "tail"],
}


def carried_values(n, seed):
    """cell_crps before the call: multiples of 2^-12 below 8."""
    return np.random.default_rng(7_000_000 + seed).integers(0, 1 << 15, n).astype(np.float64) / 4096


def assert_exact(h, y):
    """Every term of grid data is a multiple of 2^-24 and every sum over the cells (and over the
    steps, for cell_crps) stays below 2^53 such units: no float64 addition rounds, in any order."""
    tm = terms(h, y)
    x = np.float64(h.shape[0]) * tm[0] - tm[1]
    for v in (*tm, x):
        units = v / UNIT
        assert np.array_equal(units, np.round(units)), "a term off the 2^-24 grid"
        assert np.abs(units).sum() < 2.0 ** 53, "a sum past 2^53 units"
    return float(max(np.abs(v / UNIT).sum(0).max() for v in tm))


def build_case(spec):
    """-> dict(pred, row0, truth, truth_row0, t_truth0, h, y, n, M, T, thr, window keywords,
    carried or None) of a CASES entry; ``truth`` is ``pred`` itself for an aliased case."""
    n, M, T = spec["n"], spec["M"], spec["T"]
    full = spec.get("full", False)
    thr = THR4[:spec["n_thr"]]
    h = ec.make_members(n, M, T, spec["seed"], full)
    y_all = make_truth(h, spec["seed"], full)
    tb, tc = spec.get("t_begin", 0), spec.get("t_count", T - spec.get("t_begin", 0))
    if not full:
        assert_exact(h[:, :, tb:tb + tc], y_all[:, tb:tb + tc])
    if spec.get("alias"):
        pred, rows = ec.place(np.concatenate([h, y_all[None]]), spec["seed"])
        row0, truth, truth_row0, t_truth0 = rows[:M], pred, int(rows[M]), tb
    else:
        pred, row0 = ec.place(h, spec["seed"])
        t_truth0 = spec.get("t_truth0", 0)
        truth, truth_row0 = place_truth(y_all[:, tb:tb + tc], spec["seed"], spec.get("T_truth"), t_truth0)
    window = dict(t_begin=tb, t_count=tc, T_out=spec.get("T_out", tc), t_out0=spec.get("t_out0", 0))
    return dict(pred=pred, row0=row0, truth=truth, truth_row0=truth_row0, t_truth0=t_truth0, h=h, y=y_all, n=n, M=M,
                T=T, thr=thr, window=window, carried=carried_values(n, spec["seed"]) if spec.get("carried") else None)


def reference_of(c, mutant=None):
    return scores_reference(c["pred"], c["row0"], c["n"], c["truth"], c["truth_row0"], c["t_truth0"], c["thr"],
                            carried=c["carried"], mutant=mutant, **c["window"])


# ------------------------------------------------------------------ full-precision data
def sum_bounds(h, y):
    """For full-precision members ``h`` [M, n, t] and truth ``y`` [n, t]: the bound
    2 N 2^-53 sum |term| per step and sum, [t, 5], with N the number of terms of the sum --
      a      the n M differences |h_m - y|
      b      the n M (M - 1) / 2 differences |h_m - h_m'|
      |e|    the n (M + 1) addends h_m and M y
      e^2    the n (M + 1)^2 products of those addends
      v      the n M terms M h_m^2 and the n M^2 products h_m h_m' of S^2
    Each side's rounding error is at most N 2^-53 sum |term| (one rounding per term and one per
    addition, first order), hence the factor 2."""
    M, n, _ = h.shape
    hd, yd = np.abs(h.astype(np.float64)), np.abs(y.astype(np.float64))
    A = hd.sum(0) + M * yd
    tm = terms(h, y)
    mag = [tm[0].sum(0), tm[1].sum(0), A.sum(0), (A * A).sum(0), (M * (hd * hd).sum(0) + hd.sum(0) ** 2).sum(0)]
    N = [n * M, max(n * M * (M - 1) // 2, 1), n * (M + 1), n * (M + 1) ** 2, n * M * (M + 1)]
    return np.stack([2.0 * N[j] * 2.0 ** -53 * mag[j] for j in range(5)], 1)


def cell_bound(h, y):
    """The same bound for cell_crps [n]: the t M terms M |h_m - y| and the t M (M - 1) / 2 pair
    differences of a cell."""
    M, _, t = h.shape
    tm = terms(h, y)
    N = t * (M + M * (M - 1) // 2)
    return 2.0 * N * 2.0 ** -53 * (M * tm[0] + tm[1]).sum(1)


def cells_for_rounds(launch, M, T, rounds):
    """A cell count whose blocks take exactly ``rounds`` rounds of the kernel's cell loop, the last
    block ragged, from the launch query ``launch(n, M, t_count) -> (grid, cells_per_wg, iters)``:
    the smallest n (a multiple of the blocks' growth step, plus 13) that needs them."""
    n = 13
    while launch(n, M, T)[2] < rounds:
        n += 16 * 2048
    return n
