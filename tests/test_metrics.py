"""The rollout metrics without a GPU: the float64 restatement of tests/metrics_cases.py against
oracle/metrics_ref.py (itself pinned to the reference's own functions by tests/test_host_cpu.py)
on the fx_metrics fixture, the proof that the GPU comparison can fail (every mutant of the
restatement is caught by a named case), and the host side of the C ABI (the launch query, the
refusals that return before any HIP call).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import metrics_cases as mc
from conftest import golden, rel_err
from mswegnn import _lib

MSW_ERR_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def launch_query(lib):
    def launch(nrows, T):
        g, c, r, it = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        assert lib.msw_rollout_metrics_launch(nrows, T, C.byref(g), C.byref(c), C.byref(r), C.byref(it)) == _lib.MSW_OK
        return g.value, c.value, r.value, it.value
    return launch


# ------------------------------------------------------------------ the restatement
def test_restatement_reproduces_the_oracle_on_the_fixture():
    """reference + compose against oracle/metrics_ref.py and the reference's fp32 fixture.
    Losses: within the reference's own error.  Its means are fp32 accumulations; the same function
    run in float64 tells how far they are from exact arithmetic (e_ref).  The restatement differs
    from that float64 run only by taking the difference in fp32 first (2^-24 relative per term,
    twice that on a square), so |ours - fixture| <= e_ref + 2^-22 |value|.  The stacked fixture has
    no float64 twin here and keeps the 1e-5 of test_rollout_metrics_kernel_vs_reference.
    Counts, CSI and F1: equal (integers below 2^24 and one correctly rounded division: float64
    rounded once more to fp32 is the fp32 quotient, 53 >= 2 * 24 + 2)."""
    import metrics_ref as mr
    fx = golden("fx_metrics")
    n0 = int(fx["n0"])
    real_all = golden("fx_small_K4_F32_rollout48")["rollout"]
    pred_all = golden("fx_small_K2_F16_rollout48")["rollout"]
    pred, real = torch.from_numpy(pred_all[:n0]), torch.from_numpy(real_all[:n0])
    thr = (0.05, 0.3)
    ranges = [(0, n0)]
    sums, counts = mc.reference(pred_all, real_all, ranges, thr, fx["mass_area"])
    mass = dict(area=fx["mass_area"], node_bc=[fx["mass_node_bc"]], bc=[fx["mass_bc"]],
                edge_bc_length=[fx["mass_edge_bc_length"]], temporal_res=float(fx["mass_temporal_res"]))
    m = mc.compose(sums, counts, ranges, thr, mass, pred_all)
    for key, tl, water in (("rmse", "RMSE", False), ("mae", "MAE", False), ("rmse_water", "RMSE", True),
                           ("mae_water", "MAE", True)):
        want = mr.rollout_loss(pred, real, tl, water)
        assert torch.equal(want, torch.from_numpy(fx[f"loss_{tl}{'_water' if water else ''}"]))
        want64 = mr.rollout_loss(pred.double(), real.double(), tl, water).numpy()
        e_ref = np.abs(want.double().numpy() - want64)
        err = np.abs(m[key][0] - want.double().numpy())
        print(f"{key}: off the fp32 reference by {err.max():.3g}, the reference off float64 by {e_ref.max():.3g}")
        assert bool((err <= e_ref + 2.0 ** -22 * np.abs(want64)).all()), key
    for k, t in enumerate(thr):
        for i, c in enumerate(mr.confusion(pred, real, t)):
            assert np.array_equal(counts[0, :, k, i], c.numpy()), (t, i)
        for key, fn in (("csi", mr.csi), ("f1", mr.f1)):
            np.testing.assert_array_equal(m[key][t][0].astype(np.float32), fn(pred, real, t).numpy(), err_msg=key)
            np.testing.assert_array_equal(m[key][t][0].astype(np.float32), fx[f"{key}_{t}"])
    args = (torch.from_numpy(fx["mass_area"]), torch.tensor([0, n0]), torch.from_numpy(fx["mass_bc"]),
            torch.from_numpy(fx["mass_node_bc"]).long(), torch.from_numpy(fx["mass_edge_bc_length"]),
            torch.from_numpy(fx["mass_temporal_res"]))
    assert rel_err(m["mass_loss"][0], mr.mass_conservation_loss(pred, *args)) <= 1e-4
    # the stacked pair of the fixture: two simulations in one [N, 2, T] pair
    p2 = np.concatenate([pred_all[:n0], real_all[:n0, :, ::-1]])
    r2 = np.concatenate([real_all[:n0], pred_all[:n0]])
    rg2 = [(0, n0), (n0, 2 * n0)]
    m2 = mc.compose(*mc.reference(p2, r2, rg2, (0.05,)), rg2, (0.05,))
    assert rel_err(m2["rmse"], fx["loss_RMSE_stack"]) <= 1e-5
    np.testing.assert_array_equal(m2["csi"][0.05].astype(np.float32), fx["csi_0.05_stack"])


def test_grid_sums_do_not_depend_on_the_order_of_additions():
    """The premise of the bit-for-bit comparison, at the largest row count the suite uses: on grid
    data sequential, pairwise and permuted float64 sums are identical, the fp32 difference equals
    the float64 difference, and the largest sum is far below 2^53 units of 2^-24."""
    n, T = 305677, 3
    pred, real, area = mc.make_pair(n, T, 9, area=True)
    d32 = (pred - real).astype(np.float64)
    assert np.array_equal(d32, pred.astype(np.float64) - real.astype(np.float64))
    perm = np.random.default_rng(0).permutation(n)
    for term in (np.abs(d32[:, 0]), d32[:, 1] ** 2, area.astype(np.float64)[:, None] * pred[:, 0].astype(np.float64)):
        assert np.array_equal(term * 2.0 ** 24, np.round(term * 2.0 ** 24))
        pairwise = np.ascontiguousarray(term.T).sum(1)     # numpy adds a contiguous axis pairwise
        assert np.array_equal(pairwise, np.cumsum(term, 0)[-1]) and np.array_equal(pairwise, term[perm].sum(0))
        assert float(pairwise.max()) * 2.0 ** 24 < 2.0 ** 53 / 16
    # full-precision data is a different matter: the orders differ, within the bound
    pf, rf = mc.make_pair_full(20000, T, 9)
    q = (pf[:, 1] - rf[:, 1]).astype(np.float64) ** 2
    pairwise, sequential = np.ascontiguousarray(q.T).sum(1), np.cumsum(q, 0)[-1]
    assert not np.array_equal(pairwise, sequential)
    assert bool((np.abs(pairwise - sequential) <= mc.bound(pf, rf, [(0, 20000)])[0, :, 3]).all())


def test_planted_rows_are_what_they_claim():
    thr = mc.THR4
    for full in (False, True):
        pred, real = mc.make_pair(240, 9, 3, thr, full=full)
        if not full:
            for a in (pred, real):
                assert np.array_equal(a * 4096, np.round(a * 4096)) and np.abs(a).max() <= 2 and a[:, 0].min() >= 0
        dh, dv = pred[:, 0] - real[:, 0], pred[:, 1] - real[:, 1]
        kind = np.arange(240) % mc.KINDS
        assert not dh[kind == 0].any() and not dv[kind == 0].any()
        assert dh[kind == 1].all() and not dv[kind == 1].any()
        assert dv[kind == 2].all() and not dh[kind == 2].any()
        assert not dh[kind == 3].any() and np.signbit(real[kind == 3, 0]).all()
        at = np.array(thr, np.float32)[np.arange(9) % 4]
        assert (pred[kind == 4, 0] == at).all() and (real[kind == 5, 0] == at).all()
        assert (pred[kind == 6, 0] == at).all() and (real[kind == 6, 0] == at).all()
        assert (pred[kind == 7, 0] > at).all() and (real[kind == 7, 0] <= at).all()
        assert not pred[kind == 8, 0].any() and (pred[kind == 9, 0] > 1).all() and (real[kind == 9, 0] > 1).all()
        both_zero = (dh[kind >= 10] == 0) & (dv[kind >= 10] == 0)
        assert both_zero.any() and not both_zero.all()


@pytest.fixture(scope="module")
def case_results(lib):
    """(restatement, {mutant: differs}) of every named case, computed once."""
    launch = launch_query(lib)
    round_rows = launch(1 << 40, 3)[0] * launch(1 << 40, 3)[2]
    out = {}
    for name, spec in mc.CASES.items():
        c = mc.build_case(spec, launch)
        args = (c["pred"], c["real"], c["ranges"], c["thr"], c["area"])
        want = mc.reference(*args)
        out[name] = {m: mc.differs(f(*args, round_rows=round_rows), want) for m, f in mc.mutants.items()}
    return out


def test_every_mutant_is_caught_by_its_named_cases(case_results):
    """The proof that the GPU comparison can fail: each wrong variant of the restatement changes
    an asserted sum or count on the cases metrics_cases.KILLED_BY names for it, and no variant
    survives every case.  squares_in_fp32 only has to be caught on full-precision data: a grid
    case catches it too wherever a difference has more than 12 significant bits, but nothing
    relies on that."""
    assert set(mc.KILLED_BY) == set(mc.mutants)
    print()
    for m in mc.mutants:
        killers = [name for name, res in case_results.items() if res[m]]
        print(f"{m}: caught by {', '.join(killers) or 'NOTHING'}")
        assert killers, f"mutant {m} survives every case"
        for name in mc.KILLED_BY[m]:
            assert case_results[name][m], f"{name} does not catch {m}"
    full_cases = [n for n, s in mc.CASES.items() if s.get("full")]
    assert any(case_results[n]["squares_in_fp32"] for n in full_cases)


def test_mutants_are_narrow(case_results):
    """Each mutant leaves alone the cases that do not exercise its error, so a kill is evidence
    of that error and not of a broken variant."""
    spared = [("tail_rows_dropped", "full_block_256"), ("later_row_iterations_dropped", "five_sims"),
              ("steps_from_32_dropped", "row0_5"), ("ragged_time_chunk_dropped", "T64"), ("ge_for_gt", "T64"),
              ("fp_fn_swapped", "T64"), ("row0_ignored", "tail_257"), ("area_by_local_row", "tail_257"),
              ("area_by_local_row", "T65"), ("sums_leak_into_next_simulation", "tail_257")]
    for m, name in spared:
        assert not case_results[name][m], f"{m} changes {name}"


# ------------------------------------------------------------------ C ABI, host side only
@pytest.mark.parametrize("nrows, T, want", [
    (1, 32, (1, 1, 256, 1)), (256, 32, (1, 1, 256, 1)), (257, 33, (2, 2, 256, 1)),
    (131072, 32, (512, 1, 256, 1)), (131073, 33, (512, 2, 256, 2)), (305677, 3, (512, 1, 256, 3)),
    (1 << 40, 65, (512, 3, 256, 1 << 23)),
])
def test_abi_launch_values(lib, nrows, T, want):
    got = launch_query(lib)(nrows, T)
    assert got == want
    grid, _, per_wg, iters = got
    assert grid * per_wg * iters >= nrows and grid * per_wg * (iters - 1) < nrows, "iters is not minimal"


def test_abi_launch_edge_cases(lib):
    g, c, r, it = C.c_int32(7), C.c_int32(7), C.c_int32(7), C.c_int32(7)
    out = (C.byref(g), C.byref(c), C.byref(r), C.byref(it))
    for nrows, T in ((0, 8), (8, 0), (0, 0)):
        assert lib.msw_rollout_metrics_launch(nrows, T, *out) == _lib.MSW_OK
        assert (g.value, c.value, it.value) == (0, 0, 0)
    assert lib.msw_rollout_metrics_launch(-1, 8, *out) == MSW_ERR_INVALID
    assert lib.msw_rollout_metrics_launch(8, -1, *out) == MSW_ERR_INVALID
    for i in range(4):
        bad = list(out)
        bad[i] = None
        assert lib.msw_rollout_metrics_launch(8, 8, *bad) == MSW_ERR_INVALID


def _metrics(lib, pred=1, real=1, T=8, ranges=(0, 4), rng=True, num_sims=1, thr=True, n_thr=2, sums=1, counts=1):
    """msw_rollout_metrics with dummy non-NULL addresses: every call here must return before
    anything is launched, allocated or dereferenced."""
    p = lambda on: C.c_void_p(4096 if on else 0)   # noqa: E731
    return lib.msw_rollout_metrics(p(pred), p(real), T, (C.c_int64 * len(ranges))(*ranges) if rng else None, num_sims,
                                   (C.c_float * 4)(0.05, 0.3, 0, 0) if thr else None, n_thr, None, p(sums),
                                   p(counts), None)


@pytest.mark.parametrize("kw, text", [
    (dict(pred=0), "null"), (dict(real=0), "null"), (dict(rng=False), "null"), (dict(sums=0), "null"),
    (dict(thr=False), "null"), (dict(counts=0), "null"),
    (dict(n_thr=5), "n_thr"), (dict(n_thr=-1), "n_thr"), (dict(T=-1), "T"), (dict(num_sims=-1), "num_sims"),
    (dict(ranges=(4, 3)), "end < start"), (dict(ranges=(0, 4, 9, 8), num_sims=2), "end < start"),
    (dict(ranges=(-2, 4)), "negative"), (dict(ranges=(0, 1 << 31)), "int32"),
])
def test_abi_metrics_rejects_bad_arguments(lib, kw, text):
    assert _metrics(lib, **kw) == MSW_ERR_INVALID
    assert text in lib.msw_last_error().decode()


@pytest.mark.parametrize("kw", [dict(T=0), dict(T=0, num_sims=0), dict(num_sims=0), dict(T=0, thr=False, counts=0, n_thr=0)])
def test_abi_metrics_no_ops(lib, kw):
    assert _metrics(lib, **kw) == _lib.MSW_OK
