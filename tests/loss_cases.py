"""The training-loss kernels (msw_train_loss_*, csrc/loss.hip) as test cases: planted-value inputs, a
numpy float64 restatement of the forward record and of the closed-form gradient that repeats the
finalize arithmetic in the order include/mswegnn.h documents, and wrong variants ("mutants") of
that restatement, each a plausible kernel error.

A plain module (no test in it), shared by tests/test_loss.py (CPU: the restatement against
oracle/loss_ref.py in float64 and against the reference's own values in fx_loss.npz, every mutant
caught by a named case) and tests/test_gpu_loss.py (the kernels against the restatement).

Grid data (``make_rows``): every value on a 2^-12 grid with |value| <= 8, areas and BC edge lengths
small integers.  Then every d, d^2, |d| and area * (pred_h - input_h) is a multiple of 2^-24 below
2^12 and a sum over fewer than 2^17 rows stays below 2^53 of those units: each sum is exact in fp64
in ANY order, the finalize arithmetic is a fixed sequence of IEEE operations, so the kernel's record
must equal the restatement's bit for bit.  Full-precision data: the terms are still exact in fp64 (a
product of two numbers of at most 25 bits), only the order of the additions differs, and two orders
of n terms are each within (n - 1) 2^-53 sum|term| of the true sum: ``bound`` is 2 n 2^-53 sum|term|.
"""
import numpy as np

ROWS_PER_WG, MAX_WGS = 256, 512          # csrc/loss.hip: kThreads, kMaxParts
ROUND = ROWS_PER_WG * MAX_WGS            # rows of one full round of the grid-stride loop
RECORD = 12
N, SH, SV, VOL, CORR, INFLOW, CONS, LOSS, COEF_H, COEF_V, CC, DATA = range(RECORD)
KINDS = 8
SECONDS = 7200.0                         # 60 x temporal_res of the synthetic meshes (120 min)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def make_rows(n, seed, full=False):
    """-> dict(pred, real [n, 2], area, input_h [n]) float32.  Row i is of kind (i + 4) % 8:
      0  pred == real in both variables (outside mask_on_water)
      1  only h differs            2  only v differs
      3  pred h = 0 against real h = -0.0, v equal (0 - (-0.0) = 0: not water)
      4 .. 7  plain random (about a third of the random rows equal by chance in one variable)
    full=False: values on the 2^-12 grid in [-8, 8], areas integers 1..64; full=True: any fp32 value
    of the same ranges."""
    rng = np.random.default_rng(9_000_000 + seed)

    def val(lo, hi, shape):
        u = rng.random(shape) * (hi - lo) + lo
        return _f32(u if full else np.round(u * 4096) / 4096)

    real = val(-8, 8, (n, 2))
    pred = val(-8, 8, (n, 2))
    same = rng.random((n, 2)) < 0.3
    pred = np.where(same, real, pred)
    kind = (np.arange(n) + 4) % KINDS   # row 0 is a plain random row
    step = np.float32(2.0 ** -12)
    k = kind == 0
    pred[k] = real[k]
    k = kind == 1
    pred[k, 1] = real[k, 1]
    pred[k, 0] = np.where(pred[k, 0] == real[k, 0], real[k, 0] - np.sign(real[k, 0] + 0.5) * step, pred[k, 0])
    k = kind == 2
    pred[k, 0] = real[k, 0]
    pred[k, 1] = np.where(pred[k, 1] == real[k, 1], real[k, 1] - np.sign(real[k, 1] + 0.5) * step, pred[k, 1])
    k = kind == 3
    pred[k, 0], real[k, 0], pred[k, 1] = 0.0, -0.0, real[k, 1]
    area = _f32(rng.random(n) * 63 + 1 if full else rng.integers(1, 65, n))
    return dict(pred=_f32(pred), real=_f32(real), area=area, input_h=val(-8, 8, n))


def make_bc(ranges, n_rows, seed, full=False):
    """A BC list: one ghost cell inside the first non-empty range (its last row), one outside every
    range where there is such a row, and the first one again (a row listed twice) -> node_bc int64,
    bc, edge_bc_length float32."""
    rng = np.random.default_rng(9_500_000 + seed)
    inside = np.zeros(n_rows, bool)
    for s, e in ranges:
        inside[s:e] = True
    rows = [next(e - 1 for s, e in ranges if e > s)]
    outside = np.nonzero(~inside)[0]
    if len(outside):
        rows.append(int(outside[len(outside) // 2]))
    rows.append(rows[0])
    u = rng.random(len(rows)) * 4
    bc = _f32(u if full else np.round(u * 4096) / 4096)
    length = _f32(rng.random(len(rows)) * 30 + 1 if full else rng.integers(1, 32, len(rows)))
    return np.array(rows, np.int64), bc, length


def layout(sizes, gaps):
    """Row ranges of consecutive simulations of ``sizes`` fine rows, ``gaps[g]`` rows (coarse
    scales, in a real batch) before simulation g -> (ranges, total rows with a trailing gap of 3)."""
    ranges, at = [], 0
    for n, gap in zip(sizes, gaps):
        at += gap
        ranges.append((at, at + n))
        at += n
    return ranges, at + 3


def _sgn(x):
    x = np.asarray(x, np.float64)
    return np.where(x > 0, 1.0, np.where(x < 0, -1.0, x))


def _list_rows(ranges, mutant=None, round_rows=ROUND):
    """The rows of the ranges as one list, as the partial-sum launch walks them."""
    rows, pending = [], None
    for s, e in ranges:
        if mutant == "row0_ignored":
            s, e = 0, e - s
        if mutant == "leak_across_empty_range":
            # an empty range is not stepped over: the next range's rows are read from ITS start
            if e == s:
                pending = s if pending is None else pending
                continue
            if pending is not None:
                s, e, pending = pending, pending + (e - s), None
        rows.append(np.arange(s, e, dtype=np.int64))
    rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    if mutant == "tail_rows_dropped":
        rows = rows[:len(rows) // ROWS_PER_WG * ROWS_PER_WG]
    if mutant == "second_round_dropped":
        rows = rows[:round_rows]
    return rows


def restate(pred, real, ranges, type_loss="RMSE", mask=False, vs=1.0, c=0.0, num_graphs=1, area=None,
            input_h=None, node_bc=None, bc=None, length=None, seconds=SECONDS, mutant=None, round_rows=ROUND,
            abs_terms=False):
    """The forward record, float64[12] = {n, S_h, S_v, V, corr, inflow, cons, loss, coef_h, coef_v, cc,
    data}, in the operation order of include/mswegnn.h.  ``abs_terms``: every sum over |term| (the
    magnitudes ``bound`` needs)."""
    pred, real = np.asarray(pred, np.float32), np.asarray(real, np.float32)
    mae = type_loss == "MAE"
    rows = _list_rows(ranges, mutant, round_rows)
    p, r = pred[rows].astype(np.float64), real[rows].astype(np.float64)
    d = p - r
    if mutant == "mask_and":
        sel = (d[:, 0] != 0) & (d[:, 1] != 0)
    else:
        sel = (d[:, 0] != 0) | (d[:, 1] != 0)
    if not mask or mutant == "mask_ignored":
        sel = np.ones(len(rows), bool)
    term = np.abs(d) if mae else d * d
    rec = np.zeros(RECORD)
    with np.errstate(all="ignore"):
        n = float(len(rows)) if mutant == "n_over_all_rows" else float(sel.sum())
        sh, sv = float(term[sel, 0].sum() + 0.0), float(term[sel, 1].sum() + 0.0)
        on = c != 0
        vol = corr = inflow = 0.0
        if on:
            a64, in64 = np.asarray(area, np.float32).astype(np.float64), np.asarray(input_h, np.float32).astype(np.float64)
            ph = pred[:, 0].astype(np.float64)
            t = a64[rows] * (ph[rows] - in64[rows])
            vol = float((np.abs(t) if abs_terms else t).sum() + 0.0)
            nb = np.asarray(node_bc, np.int64).reshape(-1)
            nb = nb[(nb >= 0) & (nb < pred.shape[0])]
            for k in nb:   # list order
                t = a64[k] * (ph[k] - in64[k])
                corr += abs(t) if abs_terms else t
            q = 0.0
            for b, ln in zip(np.asarray(bc, np.float32).astype(np.float64), np.asarray(length, np.float32).astype(np.float64)):
                q += abs(b * ln) if abs_terms else b * ln
            inflow = q * np.float64(seconds)
        n_, sh_, sv_, vs_ = np.float64(n), np.float64(sh), np.float64(sv), np.float64(vs)
        if mutant == "sqrt_before_mean" and not mae:
            lh, lv = np.sqrt(term[sel, 0]).sum() / n_, np.sqrt(term[sel, 1]).sum() / n_
        else:
            lh, lv = (sh_ / n_, sv_ / n_) if mae else (np.sqrt(sh_ / n_), np.sqrt(sv_ / n_))
        if mutant == "velocity_scaler_on_h":
            data = (vs_ * lh + lv) / (1.0 + vs_)
        else:
            data = (lh + vs_ * lv) / (1.0 + vs_)
        G = np.float64(1 if mutant == "cons_undivided" else num_graphs)
        if mutant == "bc_correction_added":
            cons = ((np.float64(vol) - inflow) + corr) / 1e6 / G if on else np.float64(0.0)
        else:
            cons = ((np.float64(vol) - inflow) - corr) / 1e6 / G if on else np.float64(0.0)
        loss = data + np.float64(c) * np.abs(cons) if on else data
        wh, wv = 1.0 / (1.0 + vs_), vs_ / (1.0 + vs_)
        if mutant == "velocity_scaler_on_h":
            wh, wv = wv, wh
        rec[:] = (n, sh, sv, vol, corr, inflow, cons, loss,
                  wh / n_ if mae else wh / (n_ * lh), wv / n_ if mae else wv / (n_ * lv),
                  np.float64(c) * _sgn(cons) / (1e6 * G) if on else 0.0, data)
    return rec


def gradient(pred, real, ranges, rec, g=1.0, type_loss="RMSE", mask=False, c=0.0, area=None, node_bc=None,
             mutant=None):
    """grad_pred [N, 2] and grad_input_h [N] (float32) from a record, as the backward launches
    compute them (include/mswegnn.h): (float)((g * coef_c) * d) on the selected rows of the ranges,
    zeros elsewhere, the conservation part m_i = (float)((g * cc) * area_i) added in fp32 on every
    range row and taken back, in list order, at the ghost cells."""
    pred, real = np.asarray(pred, np.float32), np.asarray(real, np.float32)
    num = pred.shape[0]
    g = np.float64(np.float32(g))
    gp, gin = np.zeros((num, 2), np.float32), np.zeros(num, np.float32)
    rows = _list_rows(ranges, "row0_ignored" if mutant == "row0_ignored" else None)
    d = pred[rows].astype(np.float64) - real[rows].astype(np.float64)
    if mutant == "mask_and":
        sel = (d[:, 0] != 0) & (d[:, 1] != 0)
    else:
        sel = (d[:, 0] != 0) | (d[:, 1] != 0)
    if not mask or mutant == "mask_ignored":
        sel = np.ones(len(rows), bool)
    with np.errstate(all="ignore"):
        f = _sgn(d) if type_loss == "MAE" else d
        val = np.stack(((g * rec[COEF_H]) * f[:, 0], (g * rec[COEF_V]) * f[:, 1]), 1).astype(np.float32)
        gp[rows] = np.where(sel[:, None], val, np.float32(0))
        if c != 0:
            a64 = np.asarray(area, np.float32).astype(np.float64)
            m = ((g * rec[CC]) * a64).astype(np.float32)
            on_rows = rows[sel] if mutant == "cons_gradient_on_selected_rows" else rows
            gp[on_rows, 0] = gp[on_rows, 0] + m[on_rows]
            gin[on_rows] = -m[on_rows]
            for k in np.asarray(node_bc, np.int64).reshape(-1):
                if 0 <= k < num:
                    gp[k, 0] = gp[k, 0] - m[k]
                    gin[k] = gin[k] + m[k]
    return gp, gin


def bound(pred, real, ranges, type_loss, mask, **cons):
    """float64[4]: 2 n 2^-53 sum|term| for S_h, S_v, V (index 1..3), 0 for the exact count."""
    mag = restate(pred, real, ranges, type_loss, mask, abs_terms=True, **cons)
    n = float(sum(e - s for s, e in ranges))
    b = 2 * n * 2.0 ** -53 * np.abs(mag[:4])
    b[N] = 0.0
    return b


MUTANTS = ("mask_and", "mask_ignored", "tail_rows_dropped", "second_round_dropped", "row0_ignored",
           "leak_across_empty_range", "n_over_all_rows", "velocity_scaler_on_h", "sqrt_before_mean",
           "bc_correction_added", "cons_undivided", "cons_gradient_on_selected_rows")


def same_bits(a, b):
    """Arrays of one float type equal bit for bit, NaN matching NaN (any NaN payload)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan = np.isnan(a)
    view = np.int64 if a.dtype == np.float64 else np.int32
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(view)[~nan], b.view(view)[~nan]))


def rows_for_iterations(launch, rounds):
    """A row count that takes exactly ``rounds`` rounds of the row loop, the last one ragged (a
    third of the grid and 13 rows), from the launch query ``launch(total) -> (grid, rows_per_wg,
    iters)`` asked at a huge row count."""
    grid, per_wg, _ = launch(1 << 40)
    return grid * per_wg * (rounds - 1) + per_wg * (grid // 3) + 13


# Named cases.  sizes / gaps -> ``layout``; "iters": the row count comes from the launch query.
# cons: the mass term with conservation 0.5 and this many graphs.
CASES = {
    "one_row": dict(sizes=[1], gaps=[0], seed=1),
    "rows_255": dict(sizes=[255], gaps=[0], seed=2),
    "full_block_256": dict(sizes=[256], gaps=[0], seed=3),
    "tail_257": dict(sizes=[257], gaps=[0], seed=4),
    "rows_1499": dict(sizes=[1499], gaps=[0], seed=5),
    "row0_5": dict(sizes=[255], gaps=[5], seed=6),
    "two_iterations": dict(iters=2, gaps=[0], seed=7),
    "three_iterations": dict(iters=3, gaps=[5], seed=8),
    "empty_first": dict(sizes=[0, 300], gaps=[2, 7], seed=9),
    "empty_middle": dict(sizes=[300, 0, 257], gaps=[4, 9, 6], seed=10),
    "empty_last": dict(sizes=[17, 257, 0], gaps=[0, 131, 5], seed=11),
    "five_sims": dict(sizes=[300, 0, 1499, 17, 257], gaps=[4, 9, 0, 131, 1], seed=12),
    "cons_one": dict(sizes=[257], gaps=[5], seed=13, cons=1),
    "cons_batch3": dict(sizes=[300, 0, 257], gaps=[4, 9, 6], seed=14, cons=3),
    "full_1499": dict(sizes=[1499], gaps=[5], seed=15, full=True),
    "full_cons": dict(sizes=[700, 257], gaps=[5, 40], seed=16, full=True, cons=2),
}
OPTIONS = [(t, m, v) for t in ("RMSE", "MAE") for m in (False, True) for v in (1.0, 7.0)]

# mutant -> the named cases that must catch it (tests/test_loss.py asserts each)
KILLED_BY = {
    "mask_and": ["tail_257", "full_block_256"],
    "mask_ignored": ["tail_257", "rows_1499"],
    "tail_rows_dropped": ["one_row", "tail_257"],
    "second_round_dropped": ["two_iterations", "three_iterations"],
    "row0_ignored": ["row0_5", "five_sims"],
    "leak_across_empty_range": ["empty_first", "empty_middle"],   # five_sims: no gap after its empty range
    "n_over_all_rows": ["tail_257", "rows_255"],
    "velocity_scaler_on_h": ["tail_257", "one_row"],
    "sqrt_before_mean": ["tail_257", "rows_1499"],
    "bc_correction_added": ["cons_one", "cons_batch3"],
    "cons_undivided": ["cons_batch3", "full_cons"],
    "cons_gradient_on_selected_rows": ["cons_one", "cons_batch3"],
}


def build_case(spec, launch):
    """-> dict(pred, real, area, input_h, ranges, num_rows, full, cons) of a CASES entry; cons is {}
    or the keyword arguments of ``restate`` for the mass term."""
    sizes = spec.get("sizes") or [rows_for_iterations(launch, spec["iters"])]
    ranges, total = layout(sizes, spec["gaps"])
    full = spec.get("full", False)
    data = make_rows(total, spec["seed"], full)
    cons = {}
    if spec.get("cons"):
        nb, bc, ln = make_bc(ranges, total, spec["seed"], full)
        cons = dict(c=0.5, num_graphs=spec["cons"], area=data["area"], input_h=data["input_h"], node_bc=nb, bc=bc,
                    length=ln, seconds=SECONDS)
    return dict(pred=data["pred"], real=data["real"], area=data["area"], input_h=data["input_h"], ranges=ranges,
                num_rows=total, full=full, cons=cons)


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


def host_launch(total):
    """(grid, rows_per_wg, iters) as csrc/loss.hip picks them -- for CPU tests of this module only;
    the GPU tests ask msw_train_loss_launch."""
    if total <= 0:
        return 0, ROWS_PER_WG, 0
    blocks = -(-total // ROWS_PER_WG)
    grid = min(MAX_WGS, blocks)
    return grid, ROWS_PER_WG, -(-blocks // grid)


# ---------------------------------------------------------------- the reference's own values
def fixture_case(fx, key):
    """Inputs and options of case ``key`` ('LAYOUT/TYPE_mM_vV_cC' or 'batch/alias') of fx_loss.npz
    -> dict(pred, real, ranges, opts for restate / gradient, loss, grad, alias)."""
    lname, cname = key.split("/", 1)
    alias = cname == "alias"
    tl, m, v, c = ("RMSE", "m1", "v7", "c0.5") if alias else cname.split("_")
    c = float(c[1:])
    pred = fx[f"{lname}/preds"]
    x_h = pred[:, 0] if alias else fx[f"{lname}/x_h" if tl == "RMSE" else f"{lname}/x_h_neg"]
    cons = {}
    if c:
        cons = dict(c=c, num_graphs=int(fx[f"{lname}/num_graphs"]), area=fx[f"{lname}/area"], input_h=x_h,
                    node_bc=fx[f"{lname}/node_bc"], bc=fx[f"{lname}/bc"], length=fx[f"{lname}/edge_bc_length"],
                    seconds=60.0 * float(fx[f"{lname}/temporal_res"]))
    return dict(layout=lname, pred=pred, real=fx[f"{lname}/real"], x_h=x_h,
                ranges=[tuple(int(a) for a in r) for r in fx[f"{lname}/ranges"]], type_loss=tl, mask=m == "m1",
                vs=float(v[1:]), cons=cons, loss=fx[key + "/loss"], grad=fx[key + "/grad"], alias=alias)


def fixture_data(fx, lname, x_h, device="cpu", preds=None):
    """The ``data`` argument of loss_function for a fixture layout (mswegnn attribute bags): x with
    x[:, -2] = x_h -- or, with ``preds``, rebuilt from it as training_step does (use_prediction)."""
    import torch
    from mswegnn.batch import Batch
    from mswegnn.mesh import Graph
    from mswegnn.rollout import use_prediction
    n = fx[f"{lname}/preds"].shape[0]
    d = Batch() if bool(fx[f"{lname}/is_batch"]) else Graph()
    x = torch.zeros(n, 8)
    x[:, -2] = torch.from_numpy(np.asarray(x_h, np.float32))
    d.x = x.to(device)
    if preds is not None:
        d.x = use_prediction(d.x, preds, 3)
    d.area = torch.from_numpy(fx[f"{lname}/area"]).to(device)
    d.node_BC = torch.from_numpy(fx[f"{lname}/node_bc"]).to(device)
    d.edge_BC_length = torch.from_numpy(fx[f"{lname}/edge_bc_length"]).to(device)
    d.temporal_res = torch.tensor(int(fx[f"{lname}/temporal_res"])).to(device)
    if bool(fx[f"{lname}/has_node_ptr"]):
        r = fx[f"{lname}/ranges"]
        # the pointer of the finest scale and one coarse boundary per graph, [G, 3] or [3]
        ptr = np.concatenate((r, r[:, 1:] + 1), 1)
        d.node_ptr = torch.from_numpy(ptr if bool(fx[f"{lname}/is_batch"]) else ptr[0]).to(device)
    if bool(fx[f"{lname}/is_batch"]):
        d.num_graphs = int(fx[f"{lname}/num_graphs"])
        d.ptr = torch.zeros(d.num_graphs + 1, dtype=torch.long)
    return d, torch.from_numpy(fx[f"{lname}/bc"]).to(device)
