"""The rollout-metrics kernel (msw_rollout_metrics, csrc/metrics.hip) on the GPU against the
float64 restatement of tests/metrics_cases.py, through the C ABI.

  * grid data (metrics_cases.make_pair): every term is a multiple of 2^-24 and every sum far
    below 2^53 of those units, so each sum is exact in fp64 in any order of additions: the ten
    sums are compared BIT FOR BIT, with no tolerance.
  * full-precision data (make_pair_full): |got - want| <= 2 n 2^-53 sum|term| per sum, n the
    simulation's row count -- both sides add n terms that are exact in fp64 in some order, and
    every order is within (n - 1) 2^-53 sum|term| of the true sum: derived, not measured.  The
    largest observed ratio to it is printed when the module finishes (pytest -s).
  * counts: equal.
tests/test_metrics.py shows that the comparison can fail: every wrong variant of the
restatement (dropped tail rows, dropped loop iterations or time chunks, >= for >, ...) changes
a sum or a count on a case that also runs here (test_named_cases).
sums and counts sit between canary words; every row outside the listed ranges is poisoned (a
huge value in one run, NaN in another), so a read outside a range changes a sum.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import metrics_cases as mc
from conftest import build_msgnn, weights
from mswegnn import _lib
from mswegnn.batch import collate
from mswegnn.mesh import make_multiscale_mesh, mesh_config, wet_state
from mswegnn.metrics import finest_ranges, rollout_metrics
from mswegnn.rollout import adapt_batch_training

pytestmark = pytest.mark.gpu

PAD = 37                       # canary words on each side of both outputs
CANARY_F, CANARY_I = -12345.5, -123456789
SENTINEL = 77                  # the counts of an empty simulation: the call must leave them alone
POISONS = (7.0e8, float("nan"))
WORST = {"ratio": 0.0, "err": 0.0, "bound": 0.0, "where": ""}   # largest |got - want| / bound seen


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratio():
    yield
    print(f"\nrollout metrics, full-precision data: largest error / bound {WORST['ratio']:.3g} "
          f"(error {WORST['err']:.3g}, bound {WORST['bound']:.3g}, {WORST['where']})")


def launch(nrows, T):
    g, c, r, it = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    _lib.check(_lib.lib().msw_rollout_metrics_launch(nrows, T, C.byref(g), C.byref(c), C.byref(r), C.byref(it)))
    return g.value, c.value, r.value, it.value


def ulps(a, b):
    """Largest distance in units in the last place between two non-negative float32 tensors."""
    return int((a.contiguous().view(torch.int32).long() - b.contiguous().view(torch.int32).long()).abs().max())


class Buffers:
    """sums [S, T, 10] and counts [S, T, max(n_thr, 1), 4], each inside a canary-filled allocation.
    The sums start as canaries (the call must write every one), the counts as zeros (the call adds
    to them) -- except those of empty simulations and of a call without thresholds, which start as
    SENTINEL / canaries and must stay."""

    def __init__(self, ranges, T, n_thr, dev):
        S, K = len(ranges), max(n_thr, 1)
        self.shape_s, self.shape_c = (S, T, mc.N_SUMS), (S, T, K, 4)
        ns, nc = S * T * mc.N_SUMS, S * T * K * 4
        self.full_s = torch.full((ns + 2 * PAD,), CANARY_F, dtype=torch.float64, device=dev)
        self.full_c = torch.full((nc + 2 * PAD,), CANARY_I, dtype=torch.int64, device=dev)
        self.sums = self.full_s[PAD:PAD + ns].view(self.shape_s)
        self.counts = self.full_c[PAD:PAD + nc].view(self.shape_c)
        self.empty = [e == s for s, e in ranges]
        self.n_thr = n_thr
        if n_thr:
            self.counts.zero_()
            for g, emp in enumerate(self.empty):
                if emp:
                    self.counts[g] = SENTINEL

    def result(self):
        """-> sums, counts [S, T, n_thr, 4] as numpy, after the canary checks."""
        for b, c in ((self.full_s, CANARY_F), (self.full_c, CANARY_I)):
            assert bool((b[:PAD] == c).all()) and bool((b[-PAD:] == c).all()), "canary overwritten"
        counts = self.counts.cpu().numpy()
        if not self.n_thr:
            assert (counts == CANARY_I).all(), "counts written without thresholds"
            counts = counts[:, :, :0]
        for g, emp in enumerate(self.empty):
            if emp and self.n_thr:
                assert (counts[g] == SENTINEL).all(), f"counts of the empty simulation {g} touched"
                counts[g] = 0
        return self.sums.cpu().numpy(), counts


def call(pred, real, ranges, thr, area=None, stream=None):
    """One raw ABI call on device tensors into fresh canary buffers -> (sums, counts) as numpy."""
    T, S = pred.shape[2], len(ranges)
    bufs = Buffers(ranges, T, len(thr), pred.device)
    rng = (C.c_int64 * max(2 * S, 1))(*[v for r in ranges for v in r])
    th = (C.c_float * 4)(*(list(thr) + [0.0] * (4 - len(thr))))
    st = C.c_void_p(stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().msw_rollout_metrics(C.c_void_p(pred.data_ptr()), C.c_void_p(real.data_ptr()), T, rng, S, th,
                                              len(thr), C.c_void_p(area.data_ptr() if area is not None else 0),
                                              C.c_void_p(bufs.sums.data_ptr()), C.c_void_p(bufs.counts.data_ptr()), st))
    if stream is not None:
        torch.cuda.synchronize()
    return bufs.result()


def check(got, pred, real, ranges, thr, area, full, label):
    """got = (sums, counts) of the kernel against the restatement on the host arrays."""
    want_s, want_c = mc.reference(pred, real, ranges, thr, area)
    assert np.array_equal(got[1], want_c), f"{label}: counts"
    assert np.array_equal(got[0][..., 8], want_s[..., 8]), f"{label}: masked row count"
    if not full:
        for i in range(mc.N_SUMS):
            assert mc.same_bits(got[0][..., i], want_s[..., i]), \
                f"{label}: sum {i} off by up to {np.nanmax(np.abs(got[0][..., i] - want_s[..., i])):.3g} on grid data"
        return
    assert np.isfinite(got[0]).all(), f"{label}: sums not finite"
    err, b = np.abs(got[0] - want_s), mc.bound(pred, real, ranges, area)
    assert bool((err <= b).all()), f"{label}: sums off by up to {float((err - b).max()):.3g} over the bound"
    if (b > 0).any():
        ratio = np.where(b > 0, err / np.where(b > 0, b, 1.0), 0.0)
        at = np.unravel_index(int(ratio.argmax()), ratio.shape)
        if ratio[at] > WORST["ratio"]:
            WORST.update(ratio=float(ratio[at]), err=float(err[at]), bound=float(b[at]), where=f"{label} sum {at[2]}")


def to_dev(cuda, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def run_case(cuda, pred, real, area, ranges, thr, full, label, poisons=POISONS):
    """The call on poisoned copies (rows outside the ranges), checked against the clean arrays."""
    for value in poisons:
        p, r = mc.poison([pred, real], ranges, value)
        a = None if area is None else mc.poison([area], ranges, value)[0]
        got = call(*to_dev(cuda, p, r)[:2], ranges, thr, to_dev(cuda, a)[0])
        check(got, pred, real, ranges, thr, area, full, f"{label} poison={value}")


# ------------------------------------------------------------------ 1. shape sweep
SIZES = (1, 63, 64, 65, 255, 256, 257, 1499)


@pytest.mark.parametrize("T", [1, 3, 31, 32, 33, 64, 65])
def test_shape_sweep(cuda, T):
    """Row counts round the 64-lane wave and the 256-row workgroup, a range that starts at row 5,
    T round the 32-step time chunk, 0 / 1 / 4 thresholds, with and without area: grid data bit for
    bit, and per (nrows, row0) one full-precision run within the bound."""
    total = max(SIZES) + 5 + 3
    grid = mc.make_pair(total, T, T, area=True)
    full = mc.make_pair_full(total, T, 100 + T, area=True)
    for nrows in SIZES:
        for row0 in (0, 5):
            ranges = [(row0, row0 + nrows)]
            label = f"nrows={nrows} row0={row0} T={T}"
            dev = {}
            for value in POISONS:
                p, r, a = mc.poison(grid, ranges, value)
                dev[value] = to_dev(cuda, p, r, a)
            i = 0
            for n_thr in (0, 1, 4):
                for with_area in (True, False):
                    p, r, a = dev[POISONS[i % 2]]
                    i += 1
                    got = call(p, r, ranges, mc.THR4[:n_thr], a if with_area else None)
                    check(got, grid[0], grid[1], ranges, mc.THR4[:n_thr], grid[2] if with_area else None, False,
                          f"{label} n_thr={n_thr} area={with_area}")
            run_case(cuda, *full, ranges, mc.THR4, True, label + " full", poisons=POISONS[nrows % 2:][:1])


# ------------------------------------------------------------------ 2. the named cases (tests/test_metrics.py)
@pytest.mark.parametrize("name", list(mc.CASES))
def test_named_cases(cuda, name):
    """The cases on which tests/test_metrics.py proves that every mutant of the restatement is
    caught.  The two row-loop cases take their size from the launch query: two full rounds and a
    ragged third (about 306 k rows at T = 3, under 8 MB per tensor), and exactly two rounds."""
    spec = mc.CASES[name]
    c = mc.build_case(spec, launch)
    if "iters" in spec:
        (s, e), = c["ranges"]
        grid, chunks, per_wg, iters = launch(e - s, c["T"])
        assert iters == spec["iters"] and (e - s) % (grid * per_wg) != 0 and chunks == 1
        assert grid * per_wg * (iters - 1) < e - s <= grid * per_wg * iters
        assert c["pred"].nbytes < 8 << 20
        if spec["iters"] == 3:
            assert iters >= 3
    run_case(cuda, c["pred"], c["real"], c["area"], c["ranges"], c["thr"], c["full"], name,
             poisons=POISONS[:1] if "iters" in spec else POISONS)


# ------------------------------------------------------------------ 3. simulations
SIM_SIZES = (300, 0, 1499, 17, 257)
SIM_GAPS = (4, 9, 0, 131, 1)


@pytest.mark.parametrize("S", [1, 2, 3, 4, 5])
def test_simulations_in_one_call(cuda, S):
    """S simulations of unequal size with coarse rows between them, an empty one first, in the
    middle or last: the joint call equals the restatement, every simulation equals its own call
    bit for bit, and so does a second run."""
    T, thr = 7, mc.THR4[:3]
    for order in range(min(S, 3)):
        sizes = [int(v) for v in np.roll(SIM_SIZES[:S], order)]
        if S > 1:
            sizes[(0, S // 2, S - 1)[order]] = 0          # the empty one: first, middle, last
        ranges, total = mc.layout(sizes, SIM_GAPS[:S])
        pred, real, area = mc.make_pair(total, T, 40 + S, thr, area=True)
        label = f"S={S} sizes={sizes}"
        run_case(cuda, pred, real, area, ranges, thr, False, label)
        p, r, a = to_dev(cuda, *mc.poison([pred, real, area], ranges, POISONS[0]))
        joint = call(p, r, ranges, thr, a)
        again = call(p, r, ranges, thr, a)
        assert mc.same_bits(joint[0], again[0]) and np.array_equal(joint[1], again[1]), f"{label}: second run"
        for g, rg in enumerate(ranges):
            alone = call(p, r, [rg], thr, a)
            assert mc.same_bits(alone[0][0], joint[0][g]) and np.array_equal(alone[1][0], joint[1][g]), f"{label}: {g} alone"
            if rg[0] == rg[1]:
                assert not joint[0][g].any()
    # full-precision data: one order of the five
    ranges, total = mc.layout(SIM_SIZES[:S], SIM_GAPS[:S])
    run_case(cuda, *mc.make_pair_full(total, T, 50 + S, thr, area=True), ranges, thr, True, f"S={S} full")


def test_only_empty_simulations(cuda):
    pred, real, area = mc.make_pair(40, 5, 60, area=True)
    for ranges in ([(7, 7)], [(0, 0), (40, 40), (13, 13)]):
        for thr in (mc.THR4[:2], ()):
            got = call(*to_dev(cuda, pred, real), ranges, thr, to_dev(cuda, area)[0])
            assert got[0].shape == (len(ranges), 5, 10) and not got[0].any() and not got[1].any()


# ------------------------------------------------------------------ 4. special values
@pytest.mark.parametrize("value", [float("nan"), float("inf")])
@pytest.mark.parametrize("with_area", [True, False])
def test_one_special_value(cuda, value, with_area):
    """One NaN or +inf in a single (row, step) of pred's depth: only that simulation's sums at that
    step change, to what numpy gives (NaN or inf in the depth sums and the volume, the discharge
    sums untouched, the volume still 0 without area); NaN counts as not flooded, +inf as flooded."""
    T, thr = 9, mc.THR4
    ranges, total = mc.layout([70, 300, 65], [3, 5, 2])
    pred, real, area = mc.make_pair(total, T, 70, thr, area=True)
    area = area if with_area else None
    row, t = 336, 4                                     # a row of kind 0: pred == real there
    assert ranges[1][0] <= row < ranges[1][1] and row % mc.KINDS == 0 and pred[row, 0, t] == real[row, 0, t]
    clean = call(*to_dev(cuda, pred, real), ranges, thr, to_dev(cuda, area)[0])
    check(clean, pred, real, ranges, thr, area, False, "clean")
    bad = pred.copy()
    bad[row, 0, t] = value
    got = call(*to_dev(cuda, bad, real), ranges, thr, to_dev(cuda, area)[0])
    want_s, want_c = mc.reference(bad, real, ranges, thr, area)
    assert mc.same_bits(got[0], want_s) and np.array_equal(got[1], want_c)
    touched = np.zeros(got[0].shape[:2], bool)
    touched[1, t] = True
    assert mc.same_bits(got[0][~touched], clean[0][~touched]) and np.array_equal(got[1][~touched], clean[1][~touched])
    s = got[0][1, t]
    special = np.isnan if np.isnan(value) else np.isposinf
    assert special(s[[0, 2, 4, 6]]).all() and np.isfinite(s[[1, 3, 5, 7, 8]]).all()
    assert special(s[9]) if with_area else s[9] == 0.0
    assert s[8] == clean[0][1, t, 8] + 1                # the row entered the mask
    flooded_real = real[row, 0, t] > np.array(thr, np.float32)
    d = got[1][1, t] - clean[1][1, t]                   # [n_thr, 4]: the row moved between two cells
    for k in range(len(thr)):
        was = 0 if flooded_real[k] else 1               # pred == real before: TP or TN
        now = (0 if flooded_real[k] else 2) if np.isposinf(value) else (3 if flooded_real[k] else 1)
        want = np.zeros(4, np.int64)
        want[was] -= 1
        want[now] += 1
        assert np.array_equal(d[k], want), (k, d[k])


# ------------------------------------------------------------------ 5. base address, streams
def test_misaligned_base(cuda):
    T, n = 33, 257
    pred, real = mc.make_pair(n, T, 80)
    ranges, thr = [(0, 100), (100, n)], mc.THR4[:2]
    want = call(*to_dev(cuda, pred, real), ranges, thr)
    check(want, pred, real, ranges, thr, None, False, "aligned")
    stores = [torch.zeros(n * 2 * T + 8, device=cuda) for _ in range(2)]
    for shift in (1, 2):
        views = []
        for store, host in zip(stores, (pred, real)):
            v = store[shift:shift + n * 2 * T].view(n, 2, T)
            v.copy_(torch.from_numpy(host))
            assert v.data_ptr() % 16 == 4 * shift
            views.append(v)
        got = call(*views, ranges, thr)
        assert mc.same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]), f"shift={shift}"


@pytest.fixture(scope="module")
def engine(cuda):
    m = build_msgnn(4, 32, 4, state=weights("K4_F32")).to(cuda)
    m.engine = "hip"
    return m


def batch_graphs(T, wet=(1, None)):
    """The heterogeneous pair of the sibling suites: the tiny mesh and a 3-coarse 4-scale one."""
    tiny = make_multiscale_mesh(**mesh_config("tiny"), T=T)
    other = make_multiscale_mesh(n_coarse=3, num_scales=4, seed=5, T=T)
    return [g if w is None else wet_state(g, seed=w) for g, w in zip((tiny, other), wet)]


def test_call_behind_rollout_on_a_side_stream(cuda, engine):
    """The metrics enqueued on a non-default stream directly behind an engine rollout on that
    stream, with no host synchronisation in between (the scratch is stream-ordered
    hipMallocAsync), equal the synchronous result."""
    from mswegnn.engine import plan_for
    T, thr = 12, (0.05, 0.3)
    g = batch_graphs(T)[0].to(cuda)
    ranges = finest_ranges(g)
    whole = engine.rollout(g, T)
    real = engine.rollout(wet_state(batch_graphs(T)[0], seed=2).to(cuda), T)
    torch.cuda.synchronize()
    want = call(whole, real, ranges, thr, g.area)
    check(want, whole.cpu().numpy(), real.cpu().numpy(), ranges, thr, g.area.cpu().numpy(), True, "synchronous")
    plan = plan_for(engine, g)
    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream())
    bufs = Buffers(ranges, T, len(thr), cuda)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        out = plan.rollout(g.x, g.BC, g.node_BC, g.type_BC, T)
        _lib.check(_lib.lib().msw_rollout_metrics(
            C.c_void_p(out.data_ptr()), C.c_void_p(real.data_ptr()), T, (C.c_int64 * 2)(*ranges[0]), 1,
            (C.c_float * 4)(*thr, 0, 0), len(thr), C.c_void_p(g.area.data_ptr()), C.c_void_p(bufs.sums.data_ptr()),
            C.c_void_p(bufs.counts.data_ptr()), C.c_void_p(side.cuda_stream)))
    side.synchronize()
    assert torch.equal(out, whole)
    got = bufs.result()
    assert mc.same_bits(got[0], want[0]) and np.array_equal(got[1], want[1])


# ------------------------------------------------------------------ 6. the wrapper
def nan_equal_within_one_ulp(got, want64, label):
    """got: float32 tensor of the wrapper; want64: float64 numpy of compose.  Both sides compute
    in fp64 and round once, so only a double-rounding tie can separate them: 1 ulp."""
    got = got.cpu()
    want = torch.from_numpy(np.asarray(want64)).float()
    assert got.shape == want.shape and torch.equal(torch.isnan(got), torch.isnan(want)), f"{label}: NaN pattern"
    assert ulps(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want, nan=0.0)) <= 1, label


@pytest.mark.parametrize("name", ["tail_257", "T33", "T65", "five_sims"])
def test_wrapper_equals_compose(cuda, name):
    c = mc.build_case(mc.CASES[name], launch)
    thr = tuple(c["thr"][:3]) + (2.0,)                  # no depth is above 2: CSI and F1 undefined there
    p, r = to_dev(cuda, c["pred"], c["real"])
    m = rollout_metrics(p, r, c["ranges"], thresholds=thr)
    sums, counts = mc.reference(c["pred"], c["real"], c["ranges"], thr)
    want = mc.compose(sums, counts, c["ranges"], thr)
    assert np.array_equal(m["counts"].cpu().numpy()[:, :, :len(thr)], counts)
    for k in ("rmse", "mae", "rmse_water", "mae_water"):
        nan_equal_within_one_ulp(m[k], want[k], f"{name}: {k}")
    none_flooded = counts[..., :1].sum(-1) + counts[..., 2:].sum(-1) == 0    # TP + FP + FN
    for k in ("csi", "f1"):
        assert set(m[k]) == {float(t) for t in thr}
        for i, t in enumerate(thr):
            nan_equal_within_one_ulp(m[k][float(t)], want[k][float(t)], f"{name}: {k}[{t}]")
            assert np.array_equal(torch.isnan(m[k][float(t)]).cpu().numpy(), none_flooded[:, :, i]), (k, t)
        assert bool(torch.isnan(m[k][2.0]).all())
    nonempty = np.array([e > s for s, e in c["ranges"]])
    assert not bool(torch.isnan(m["csi"][float(thr[0])]).cpu()[torch.from_numpy(nonempty)].all())
    # an empty simulation: NaN losses, no exception
    for g, (s, e) in enumerate(c["ranges"]):
        if s == e:
            assert all(bool(torch.isnan(m[k][g]).all()) for k in ("rmse", "mae", "rmse_water", "mae_water"))
    # pred == real: the masked losses are 0 / 0
    same = rollout_metrics(p, p, c["ranges"], thresholds=thr[:1])
    assert bool(torch.isnan(same["rmse_water"]).all()) and bool(torch.isnan(same["mae_water"]).all())
    assert not bool(same["rmse"][torch.from_numpy(nonempty)].any())
    # fp64 and non-contiguous inputs
    wide = torch.zeros(p.shape[0], 2, 2 * p.shape[2], device=cuda, dtype=torch.float64)
    wide[:, :, ::2] = p
    other = rollout_metrics(wide[:, :, ::2], r.double(), c["ranges"], thresholds=thr)
    assert not wide[:, :, ::2].is_contiguous()
    for k in ("rmse", "mae", "rmse_water", "mae_water"):
        assert torch.equal(torch.nan_to_num(other[k], nan=-7.0), torch.nan_to_num(m[k], nan=-7.0)), k
    assert torch.equal(other["counts"], m["counts"])


def _mass_args(b, gs):
    S = len(gs)
    return dict(area=b.area, node_bc=[b.node_BC[b.node_BC_ptr.to(b.node_BC.device) == g] for g in range(S)],
                bc=[g.BC[:, -1, :] for g in gs], edge_bc_length=[g.edge_BC_length[:1] for g in gs],
                temporal_res=float(b.temporal_res))


def test_mass_loss_with_two_simulations(cuda):
    """mass['node_bc'][g] holds GRAPH rows: for a batch, node_BC as adapt_batch_training leaves it
    (ptr[g] + the simulation's own node_BC, the reference's training/train.py:18).  The reference
    evaluates get_mass_conservation_loss one simulation at a time on its finest rows, where
    conservation_loss indexes (area * delta_WD)[data.node_BC] with the simulation's own numbering
    (training/loss.py:161) -- the same cells.  So mass_loss[g] of the batch equals
    metrics_ref.mass_conservation_loss on simulation g's finest rows alone, within the 1e-4 of the
    largest that the fixture test uses (fp64 sums against the reference's fp32 sums).  Rows
    outside simulation g's finest range are refused: the simulation's own numbering, passed by
    mistake for g > 0, then fails loudly wherever it leaves that range (it cannot when the row
    happens to lie inside it, which is why the numbering is documented)."""
    import metrics_ref as mr
    from conftest import rel_err
    T = 12
    gs = batch_graphs(T + 1)
    b = adapt_batch_training(collate(gs))
    ranges = finest_ranges(b)
    assert ranges[1][0] > ranges[0][1] > 0               # coarse rows of simulation 0 in between
    pred, real = mc.make_pair(b.x.shape[0], T, 90)
    mass = _mass_args(b, gs)
    for g in range(2):
        assert int(mass["node_bc"][g]) == int(b.ptr[g]) + int(gs[g].node_BC) and gs[g].BC.shape[-1] >= T + 1
    m = rollout_metrics(*to_dev(cuda, pred, real), ranges, mass=mass)
    sums, counts = mc.reference(pred, real, ranges, (0.05, 0.3), b.area.numpy())
    want = mc.compose(sums, counts, ranges, (0.05, 0.3), {k: v for k, v in mass.items()}, pred)
    for g, (s, e) in enumerate(ranges):
        ref = mr.mass_conservation_loss(torch.from_numpy(pred[s:e]), gs[g].area, gs[g].node_ptr, gs[g].BC[:, -1, :],
                                        gs[g].node_BC.long(), gs[g].edge_BC_length[:1], gs[g].temporal_res)
        assert ref.shape == (T - 1,) and float(ref.abs().max()) > 0
        assert rel_err(m["mass_loss"][g].cpu(), ref) <= 1e-4, g
        assert rel_err(m["mass_loss"][g].cpu(), want["mass_loss"][g]) <= 2.0 ** -22, g
    # the comparison tells the numberings apart: simulation 1's own numbering reads simulation 0's cells
    local = dict(mass, node_bc=[g.node_BC for g in gs])
    wrong = mc.compose(sums, counts, ranges, (0.05, 0.3), local, pred)["mass_loss"][1]
    assert rel_err(wrong, want["mass_loss"][1]) > 1e-4
    assert ranges[1][0] <= int(gs[1].node_BC) < ranges[1][1]        # here it stays inside: no refusal possible
    outside = dict(mass, node_bc=[mass["node_bc"][0], mass["node_bc"][0]])
    with pytest.raises(ValueError, match="graph rows"):
        rollout_metrics(*to_dev(cuda, pred, real), ranges, mass=outside)


# ------------------------------------------------------------------ 7. the engine, end to end
def test_engine_rollout_of_a_batch(cuda, engine):
    """A heterogeneous batch rolled out on the HIP engine against a second rollout (other initial
    states) as ``real``: per simulation the metrics of the batch equal those of the graph rolled
    out alone, and the reference's evaluation (oracle/metrics_ref.py, fp32) on the CPU copies --
    losses within the reference's own distance from float64 arithmetic plus 2^-22 relative (the
    fp32 difference taken first), CSI and F1 equal."""
    import metrics_ref as mr
    T, thr = 12, (0.05, 0.3)
    gp, gr = batch_graphs(T, (1, None)), batch_graphs(T, (2, 3))
    bp, br = (adapt_batch_training(collate(gs)).to(cuda) for gs in (gp, gr))
    steps0 = _plan_steps(engine, bp)
    pred, real = engine.rollout(bp, T), engine.rollout(br, T)
    assert _plan_steps(engine, bp) >= steps0 + T         # the HIP path ran them
    ranges = finest_ranges(bp)
    assert len(ranges) == 2 and ranges[1][0] > ranges[0][1]
    m = rollout_metrics(pred, real, ranges, thresholds=thr)
    ph, rh = pred.cpu(), real.cpu()
    raw = call(pred.contiguous(), real.contiguous(), ranges, thr)    # the sums, which the wrapper does not return
    assert np.array_equal(raw[1], m["counts"].cpu().numpy())
    check(raw, ph.numpy(), rh.numpy(), ranges, thr, None, True, "batch")
    for g, (s, e) in enumerate(ranges):
        a, b = gp[g].to(cuda), gr[g].to(cuda)
        alone = rollout_metrics(engine.rollout(a, T), engine.rollout(b, T), finest_ranges(a), thresholds=thr)
        for k in ("rmse", "mae", "rmse_water", "mae_water"):
            assert torch.equal(alone[k][0], m[k][g]), (g, k)
        assert torch.equal(alone["counts"][0], m["counts"][g])
        p, r = ph[s:e], rh[s:e]
        assert float((p - r).abs().max()) > 1e-3         # the two rollouts really differ
        for k, tl, water in (("rmse", "RMSE", False), ("mae", "MAE", False), ("rmse_water", "RMSE", True),
                             ("mae_water", "MAE", True)):
            ref32 = mr.rollout_loss(p, r, tl, water).double()
            ref64 = mr.rollout_loss(p.double(), r.double(), tl, water)
            err = (m[k][g].cpu().double() - ref32).abs()
            assert bool((err <= (ref32 - ref64).abs() + 2.0 ** -22 * ref64.abs()).all()), (g, k, err, ref32 - ref64)
        for t in thr:
            for k, fn in (("csi", mr.csi), ("f1", mr.f1)):
                want = fn(p, r, t)
                assert torch.equal(torch.nan_to_num(m[k][t][g].cpu(), nan=-7.0), torch.nan_to_num(want, nan=-7.0)), (g, k, t)


def _plan_steps(m, g):
    from mswegnn.engine import plan_for
    return plan_for(m, g).stats()["rollout_steps"]


# ------------------------------------------------------------------ 8. fuzz
def _seeds():
    a, b = (int(v) for v in os.environ.get("METRICS_FUZZ_SEEDS", "0:12").split(":"))
    return range(a, b)


def draw(seed):
    rng = np.random.default_rng(50_000 + seed)
    S = int(rng.integers(1, 6))
    sizes = [int(rng.choice([0, 1, int(rng.integers(2, 300)), int(rng.integers(300, 3001))], p=[0.1, 0.1, 0.4, 0.4]))
             for _ in range(S)]
    n_thr = int(rng.integers(0, 5))
    return dict(sizes=sizes, gaps=[int(v) for v in rng.integers(0, 41, S)], T=int(rng.integers(1, 81)),
                thr=tuple(float(v) for v in rng.permutation(mc.THR4)[:n_thr]), area=bool(rng.random() < 0.5),
                full=bool(rng.random() < 0.5))


@pytest.mark.parametrize("seed", _seeds())
def test_random_cases(cuda, seed):
    """METRICS_FUZZ_SEEDS="a:b" widens the seed range (default 0:12) for a longer sweep."""
    c = draw(seed)
    ranges, total = mc.layout(c["sizes"], c["gaps"])
    pred, real, area = mc.make_pair(total, c["T"], 1000 + seed, c["thr"], area=True, full=c["full"])
    run_case(cuda, pred, real, area if c["area"] else None, ranges, c["thr"], c["full"], f"seed={seed} {c}",
             poisons=POISONS[seed % 2:][:1])
