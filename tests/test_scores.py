"""The ensemble scores on the CPU: ``mswegnn.ensemble``'s torch path against the independent numpy
restatement of tests/scores_cases.py (bit for bit on grid data), every wrong variant of the
restatement caught by a named case, the identities that tie the sums to the CRPS and the Brier
score, the chunked driver on the torch path, and the C ABI's refusals and launch query (host side:
they return before any HIP call).  The reference has no counterpart for these scores."""
import ctypes as C

import numpy as np
import pytest
import torch

import ensemble_cases as ec
import scores_cases as sc
from conftest import build_msgnn, weights
from mswegnn import _lib
from mswegnn import ensemble as ens
from mswegnn.ensemble import EnsembleScores, ensemble_scores, make_ensemble, member_ranges, rollout_ensemble
from mswegnn.mesh import hydrograph_bc, make_multiscale_mesh, mesh_config, wet_state


@pytest.fixture(scope="module")
def cases():
    return {name: sc.build_case(spec) for name, spec in sc.CASES.items()}


def ranges_of(c):
    return [(int(r), int(r) + c["n"]) for r in c["row0"]]


# ------------------------------------------------------------------ the torch path == the restatement
@pytest.mark.parametrize("name", sc.GRID_CASES)
def test_torch_equals_restatement(cases, name):
    c = cases[name]
    w = c["window"]
    tb, tc = w["t_begin"], w["t_count"]
    want = sc.reference_of(c)
    pred, truth = torch.from_numpy(c["pred"]), torch.from_numpy(c["truth"])
    y = truth[c["truth_row0"]:c["truth_row0"] + c["n"], 0, c["t_truth0"]:c["t_truth0"] + tc]
    got = ens._scores_torch(pred[:, :, tb:tb + tc], [int(r) for r in c["row0"]], c["n"], y, c["thr"])
    at = slice(w["t_out0"], w["t_out0"] + tc)
    assert np.array_equal(got["sums"].numpy(), want["sums"][at])
    assert np.array_equal(got["reliability"].numpy(), want["reliability"][at])
    # the class: the window lands in the next columns and onto the carried cell_crps
    es = EnsembleScores(ranges_of(c), tc + 1, c["thr"])
    es.update(pred, truth, tb, 1, c["truth_row0"], c["t_truth0"])
    first = es.arrays["cell_crps"].clone()
    es.arrays["cell_crps"].copy_(torch.from_numpy(np.zeros(c["n"]) if c["carried"] is None else c["carried"]))
    es.update(pred, truth, tb, tc, c["truth_row0"], c["t_truth0"])
    assert es.steps_seen == tc + 1
    assert np.array_equal(es.arrays["sums"][1:].numpy(), want["sums"][at])
    assert np.array_equal(es.arrays["sums"][0].numpy(), want["sums"][w["t_out0"]])
    assert np.array_equal(es.arrays["reliability"][1:].numpy(), want["reliability"][at])
    assert np.array_equal(es.arrays["cell_crps"].numpy(), want["cell_crps"])
    one = sc.scores_reference(c["pred"], c["row0"], c["n"], c["truth"], c["truth_row0"], c["t_truth0"], c["thr"], tb, 1)
    assert np.array_equal(first.numpy(), one["cell_crps"])


def test_result_divides_the_sums(cases):
    c = cases["tail"]
    M, n, T = c["M"], c["n"], c["T"]
    res = ensemble_scores(torch.from_numpy(c["pred"]), torch.from_numpy(c["truth"]), ranges_of(c), c["thr"],
                          truth_row0=c["truth_row0"])
    want = sc.scores_reference(c["pred"], c["row0"], n, c["truth"], c["truth_row0"], 0, c["thr"])
    s = want["sums"]
    assert res["steps"] == T and res["members"] == M and np.array_equal(res["sums"].numpy(), s)
    assert np.array_equal(res["crps"].numpy(), s[:, 0] / (M * n) - s[:, 1] / (M * M * n))
    assert np.isclose(float(res["crps_mean"]), res["crps"].numpy().mean(), rtol=1e-15)
    assert np.array_equal(res["mae_mean"].numpy(), s[:, 2] / (M * n))
    assert np.array_equal(res["rmse_mean"].numpy(), np.sqrt(s[:, 3] / (M * M * n)))
    assert np.array_equal(res["spread"].numpy(), np.sqrt(s[:, 4] / (M * M * n)))
    assert np.array_equal(res["spread_skill"].numpy(), res["spread"].numpy() / res["rmse_mean"].numpy())
    assert np.array_equal(res["cell_crps"].numpy(), want["cell_crps"] / (M * M * T))
    assert set(res["reliability"]) == set(res["brier"]) == set(float(np.float64(t)) for t in c["thr"])
    for k, t in enumerate(c["thr"]):
        r = res["reliability"][t]
        assert np.array_equal(r["forecast_prob"].numpy(), np.arange(M + 1) / M)
        assert np.array_equal(r["n"].numpy(), want["reliability"][:, k, :, 0])
        assert np.array_equal(r["observed"].numpy(), want["reliability"][:, k, :, 1])
        assert (r["n"].sum(1) == n).all()
    only = ensemble_scores(torch.from_numpy(c["pred"]), torch.from_numpy(c["truth"]), ranges_of(c), c["thr"],
                           want=("sums",), truth_row0=c["truth_row0"])
    assert "reliability" not in only and "cell_crps" not in only and torch.equal(only["sums"], res["sums"])


def test_argument_errors(cases):
    c = cases["m3"]
    pred, r = torch.from_numpy(c["pred"]), ranges_of(c)
    ok = dict(truth=pred, truth_row0=c["truth_row0"], truth_t0=0)
    with pytest.raises(ValueError):
        EnsembleScores(r, 5, want=("crps",))
    with pytest.raises(ValueError):
        EnsembleScores(r, 5, thresholds=(0.1,) * 5)
    with pytest.raises(ValueError):
        EnsembleScores([(0, 4), (4, 9)], 5)
    for kw in (dict(t_begin=-1), dict(t_begin=3, t_count=3), dict(truth_t0=1), dict(truth_t0=-1),
               dict(truth_row0=-1), dict(truth_row0=pred.shape[0] - 3), dict(truth=pred[:, :1]), dict(truth=pred[0])):
        with pytest.raises(ValueError):
            EnsembleScores(r, 5).update(pred, **{**ok, **kw})
    with pytest.raises(ValueError):
        EnsembleScores(r, 4).update(pred, **ok)              # more steps than the arrays hold
    with pytest.raises(ValueError):
        EnsembleScores(r, 5).update(pred[:10], **ok)
    with pytest.raises(ValueError):
        EnsembleScores(r, 5).update(pred[:, 0], **ok)


# ------------------------------------------------------------------ every mutant is caught
@pytest.mark.parametrize("mutant", list(sc.KILLED_BY))
def test_mutants_are_caught(cases, mutant):
    for name in sc.KILLED_BY[mutant]:
        assert not sc.same(sc.reference_of(cases[name], mutant), sc.reference_of(cases[name])), name


def test_every_mutant_is_listed():
    assert set(sc.KILLED_BY) == set(sc.MUTANTS) and all(sc.KILLED_BY.values())
    assert all(set(v) <= set(sc.CASES) for v in sc.KILLED_BY.values())
    assert {sc.CASES[k]["n"] for k in sc.KILLED_BY["tail_dropped"]} == {65, 257}


def test_planted_truths(cases):
    c = cases["tail"]
    h, y, thr = c["h"], c["y"], np.array(sc.THR4, np.float32)
    kind = (np.arange(c["n"]) // 2) % sc.TRUTH_KINDS
    t = np.arange(c["T"])
    assert (y[kind == 0] == h[0, kind == 0]).all() and (y[kind == 1] == 0).all()
    assert (y[kind == 2] == thr[t % 4]).all() and (y[kind == 3] != thr[t % 4]).all()
    assert (np.abs(y[kind == 3] - thr[t % 4]) <= np.float32(sc.STEP)).all()
    assert (y[kind == 4] > h[:, kind == 4]).all()
    below = y[kind == 5][None] < h[:, kind == 5]
    assert (below | (h[:, kind == 5] == 0)).all()
    assert np.isnan(c["truth"][:, 1]).all() and c["truth_row0"] > 0
    assert sc.assert_exact(h, y) < 2.0 ** 53 / 100         # a wide margin below 2^53 units
    big = ec.make_members(1499, 64, 8, 3)                   # the GPU sweep's largest grid case
    assert sc.assert_exact(big, sc.make_truth(big, 3)) < 1e14


# ------------------------------------------------------------------ identities
def test_one_member_and_perfect_ensemble(cases):
    c = cases["m1"]
    got = sc.reference_of(c)
    assert got["sums"][0, 1] == 0 and got["sums"][0, 0] == abs(np.float64(c["h"][0, 0, 0]) - np.float64(c["y"][0, 0]))
    h = ec.make_members(40, 5, 6, 9)
    h[:] = h[:1]
    pred, row0 = ec.place(np.concatenate([h, h[:1]]), 9)
    res = ensemble_scores(torch.from_numpy(pred), torch.from_numpy(pred), [(int(r), int(r) + 40) for r in row0[:5]],
                          truth_row0=int(row0[5]))
    assert not res["sums"].any() and not res["cell_crps"].any() and not res["crps"].any()


def test_pair_sum_equals_the_sorted_formula(cases):
    for name in sc.GRID_CASES:
        c = cases[name]
        h = c["h"].astype(np.float64)
        M = c["M"]
        coef = (2 * np.arange(1, M + 1) - M - 1)[:, None, None]
        assert np.array_equal((coef * np.sort(h, 0)).sum(0), sc.terms(c["h"], c["y"])[1]), name


def test_crps_is_the_integral_of_the_squared_cdf_difference(cases):
    c = cases["full_m7"]
    h, y, M = c["h"].astype(np.float64), c["y"].astype(np.float64), c["M"]
    tm = sc.terms(c["h"], c["y"])
    crps = tm[0] / M - tm[1] / (M * M)
    for i in range(0, c["n"], 3):
        for t in (0, 17, 47):
            x = np.sort(np.concatenate([h[:, i, t], [y[i, t]]]))
            mid = (x[1:] + x[:-1]) / 2
            F = (h[:, i, t][None, :] <= mid[:, None]).mean(1)
            integral = (((F - (y[i, t] <= mid)) ** 2) * np.diff(x)).sum()
            assert abs(integral - crps[i, t]) < 1e-12


def test_brier_from_the_table(cases):
    c = cases["tail"]
    res = ensemble_scores(torch.from_numpy(c["pred"]), torch.from_numpy(c["truth"]), ranges_of(c), c["thr"],
                          truth_row0=c["truth_row0"])
    for t in c["thr"]:
        p = (c["h"] > np.float32(t)).sum(0) / c["M"]
        want = ((p - (c["y"] > np.float32(t))) ** 2).mean(0)
        assert np.abs(res["brier"][t].numpy() - want).max() < 1e-12


def test_nan_depths(cases):
    c = cases["m3"]
    pred = c["pred"].copy()
    n, T = c["n"], c["T"]
    pred[c["row0"][1] + 7, 0, 2] = np.nan          # a member: cell 7, step 2
    pred[c["truth_row0"] + 11, 0, 4] = np.nan      # the truth: cell 11, step 4
    es = EnsembleScores(ranges_of(c), T, c["thr"]).update(torch.from_numpy(pred), torch.from_numpy(pred),
                                                          truth_row0=c["truth_row0"])
    res = es.result()
    want = sc.scores_reference(pred, c["row0"], n, pred, c["truth_row0"], 0, c["thr"])
    clean = sc.scores_reference(c["pred"], c["row0"], n, c["pred"], c["truth_row0"], 0, c["thr"])
    assert np.array_equal(res["sums"].numpy(), want["sums"], equal_nan=True)
    assert np.isnan(want["sums"][[2, 4]]).all() and np.array_equal(want["sums"][[0, 1, 3]], clean["sums"][[0, 1, 3]])
    assert list(np.nonzero(np.isnan(want["cell_crps"]))[0]) == [7, 11]
    assert np.array_equal(es.arrays["cell_crps"].numpy(), want["cell_crps"], equal_nan=True)
    assert np.array_equal(np.isnan(res["cell_crps"].numpy()), np.isnan(want["cell_crps"]))
    assert (want["reliability"].sum(2)[..., 0] == n).all()
    for k, t in enumerate(c["thr"]):
        assert np.array_equal(res["reliability"][t]["n"].numpy(), want["reliability"][:, k, :, 0])
        assert np.array_equal(res["reliability"][t]["observed"].numpy(), want["reliability"][:, k, :, 1])


# ------------------------------------------------------------------ the driver
@pytest.fixture(scope="module")
def tiny_model():
    return build_msgnn(num_scales=4, hid=32, K=4, state=weights("K4_F32"))


@pytest.fixture(scope="module")
def tiny_ensemble():
    g = wet_state(make_multiscale_mesh(**mesh_config("tiny"), T=9), seed=1)
    bcs = [hydrograph_bc(9, peak=p, seed=s) for p, s in ((1.0, 1), (3.0, 2), (6.0, 3), (2.0, 4))]
    return make_ensemble(g, bcs)


def _same(u, v):
    if isinstance(u, dict):
        return u.keys() == v.keys() and all(_same(u[k], v[k]) for k in u)
    if not isinstance(u, torch.Tensor):
        return u == v
    if torch.is_floating_point(u):
        u, v = torch.nan_to_num(u, nan=-7.0), torch.nan_to_num(v, nan=-7.0)
    return u.dtype == v.dtype and torch.equal(u, v)


def test_rollout_ensemble_with_truth(tiny_model, tiny_ensemble):
    b = tiny_ensemble
    ranges = member_ranges(b)
    members, control = ranges[:3], ranges[3]       # the fourth run is the truth, not a member
    n = control[1] - control[0]
    whole, rw = rollout_ensemble(tiny_model, b, 9, chunk=None, keep_rollout=True)
    assert set(whole) == {"maps", "steps"}                       # without a truth: the keys it has always had
    truth = rw[control[0]:control[1]].clone()
    scored, _ = rollout_ensemble(tiny_model, b, 9, chunk=None, keep_rollout=True, truth=truth)
    assert set(scored) == {"maps", "steps", "scores"}
    assert _same(scored["maps"], whole["maps"]) and _same(scored["steps"], whole["steps"])
    for chunk in (4, 1):
        parts = rollout_ensemble(tiny_model, b, 9, chunk=chunk, truth=truth)
        assert _same(parts["scores"], scored["scores"]), chunk
        rows = rollout_ensemble(tiny_model, b, 9, chunk=chunk, truth=rw, truth_row0=control[0])
        assert _same(rows["scores"], scored["scores"]), chunk
    s = scored["scores"]
    assert s["steps"] == 9 and s["members"] == 4 and bool((s["crps"] > 0).any()) and bool((s["spread"] > 0).any())
    direct = ensemble_scores(rw, truth, ranges)
    assert _same(direct, s)
    # three members against the control run, chunked by hand: the bits of the whole
    one = ensemble_scores(rw, rw, members, truth_row0=control[0])
    es = EnsembleScores(members, 9)
    for t0 in range(0, 9, 4):
        es.update(rw, rw, t0, min(4, 9 - t0), truth_row0=control[0])
    assert _same(es.result(), one)
    want = sc.scores_reference(rw.numpy(), [s0 for s0, _ in members], n, rw.numpy(), control[0], 0, (0.05, 0.3))
    bound = sc.sum_bounds(ec.gather(rw.numpy(), [s0 for s0, _ in members], n), rw.numpy()[control[0]:control[1], 0])
    assert (np.abs(one["sums"].numpy() - want["sums"]) <= bound).all()
    assert np.array_equal(one["reliability"][0.05]["n"].numpy(), want["reliability"][:, 0, :, 0])


# ------------------------------------------------------------------ C ABI, host side only
@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def test_struct_size_and_abi(lib):
    assert lib.msw_struct_size(b"msw_ensemble_scores_out") == C.sizeof(_lib.MswEnsembleScoresOut) == 24
    assert lib.msw_abi_version() == 1
    names = [s[0] for s in _lib.SYMBOLS]
    assert "msw_ensemble_scores_update" in names and "msw_ensemble_scores_launch" in names
    assert _lib.STRUCTS["msw_ensemble_scores_out"] is _lib.MswEnsembleScoresOut


class HostCanaries:
    """Host arrays handed over as if they were device memory: a refused call returns before
    anything is launched or dereferenced, so they must keep their canaries."""

    def __init__(self):
        self.pred = np.full(4096, ec.CANARY_F, np.float32)
        self.sums = np.full(8 * 5, sc.CANARY_D, np.float64)
        self.table = np.full(8 * 2 * 3 * 2, sc.CANARY_L, np.int64)
        self.cell = np.full(4, sc.CANARY_D, np.float64)

    def untouched(self):
        return bool((self.pred == ec.CANARY_F).all() and (self.sums == sc.CANARY_D).all() and
                    (self.table == sc.CANARY_L).all() and (self.cell == sc.CANARY_D).all())


def scores_call(lib, hc, pred=True, truth=True, T=8, t_begin=0, t_count=8, rows=(0, 10), M=None, n=4, Tt=8, tt0=0, trow0=20,
                thr=True, n_thr=2, T_out=8, t_out0=0, out=True, row0=True, outputs=("sums", "reliability", "cell_crps")):
    ptr = {"sums": hc.sums.ctypes.data, "reliability": hc.table.ctypes.data, "cell_crps": hc.cell.ctypes.data}
    o = _lib.MswEnsembleScoresOut(**{k: ptr[k] for k in outputs})
    th = (C.c_float * 4)(0.05, 0.3, 0, 0)
    r = (C.c_int64 * 65)(*rows)
    p = C.c_void_p(hc.pred.ctypes.data)
    return lib.msw_ensemble_scores_update(p if pred else None, T, t_begin, t_count, r if row0 else None,
                                          len(rows) if M is None else M, n, p if truth else None, Tt, tt0, trow0,
                                          th if thr else None, n_thr, T_out, t_out0, C.byref(o) if out else None, None)


REFUSED = [
    (dict(pred=False), "null"), (dict(truth=False), "null"), (dict(out=False), "null"), (dict(row0=False), "null"),
    (dict(thr=False), "null"), (dict(M=0), "M out"), (dict(M=65), "M out"), (dict(M=-1), "M out"),
    (dict(n_thr=5), "n_thr"), (dict(n_thr=-1), "n_thr"), (dict(n=-1), "n negative"), (dict(rows=(0, -1)), "member_row0"),
    (dict(trow0=-1), "truth_row0"), (dict(t_begin=-1), "window"), (dict(t_begin=4, t_count=5), "window"),
    (dict(t_count=-1), "window"), (dict(T=-1, t_count=0), "window"), (dict(tt0=-1), "truth columns"),
    (dict(tt0=1), "truth columns"), (dict(Tt=7), "truth columns"), (dict(t_out0=-1), "output columns"),
    (dict(t_out0=1), "output columns"), (dict(T_out=7), "output columns"),
]


@pytest.mark.parametrize("kw, text", REFUSED)
def test_abi_rejects_bad_arguments(lib, kw, text):
    hc = HostCanaries()
    assert scores_call(lib, hc, **kw) == -1  # MSW_ERR_INVALID
    assert text in lib.msw_last_error().decode()
    assert hc.untouched()


def test_abi_no_ops(lib):
    hc = HostCanaries()
    for kw in (dict(t_count=0), dict(n=0), dict(outputs=()), dict(outputs=("reliability",), n_thr=0, thr=False),
               dict(t_count=0, T_out=0, Tt=0)):
        assert scores_call(lib, hc, **kw) == _lib.MSW_OK, kw
    assert hc.untouched()


@pytest.mark.parametrize("t_count", [1, 4, 47, 48, 257])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 10369, 1 << 33])
def test_abi_launch_is_consistent(lib, n, t_count):
    for M in (1, 16, 17, 64):
        g, r, it = ens.scores_launch(n, M, t_count)
        assert g >= 1 and it >= 1 and 1 <= r <= 64
        assert g * r * it >= n
        assert (g - 1) * r * (it - 1) < n, "more blocks or rounds than the cells need"
        # the blocks -- the order of the sums -- depend on n alone
        assert g == ens.scores_launch(n, 1, 1)[0] == -(-n // ens._block_cells(n))
    if n < 1 << 20:
        assert EnsembleScores([(0, n)] * 3, 1).launch(t_count) == ens.scores_launch(n, 3, t_count)


def test_abi_launch_edge_cases(lib):
    assert ens.scores_launch(0, 4, 8)[::2] == (0, 0) and ens.scores_launch(8, 4, 0)[::2] == (0, 0)
    g, r, it = C.c_int32(), C.c_int32(), C.c_int32()
    for n, M, t in ((-1, 4, 8), (8, 4, -1), (8, 0, 8), (8, 65, 8)):
        assert lib.msw_ensemble_scores_launch(n, M, t, C.byref(g), C.byref(r), C.byref(it)) == -1
    assert lib.msw_ensemble_scores_launch(8, 4, 8, None, C.byref(r), C.byref(it)) == -1
    # the blocks grow with n in steps of 16 cells, 2048 of them at most up to 2^26 cells
    assert [ens._block_cells(n) for n in (1, 32768, 32769, 65536, 65537, 1 << 26, 1 << 33)] == \
        [16, 16, 32, 32, 48, 32768, 32768]
