"""The ensemble-scores kernel (msw_ensemble_scores_update) on the GPU against the numpy restatement
of tests/scores_cases.py -- the reference has no counterpart.  On the planted 2^-12 grid data every
term and every sum is exact in float64 (the case builder asserts it), so sums, table and cell_crps
are compared bit for bit; on full-precision data the sums lie within 2 N 2^-53 sum |term| of the
restatement, and a horizon scored in chunks still gives the bits of one call.  Every output sits
between canary words, columns outside a call's window keep theirs, and the rows around every
member range and the truth range hold NaN or 7e8.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import ensemble_cases as ec
import scores_cases as sc
from conftest import build_msgnn, weights
from mswegnn import _lib
from mswegnn.ensemble import (EnsembleScores, ensemble_scores, make_ensemble, member_ranges, rollout_ensemble,
                              scores_launch)
from mswegnn.mesh import hydrograph_bc, make_multiscale_mesh, mesh_config

pytestmark = pytest.mark.gpu

PAD = 37  # canary words on each side of every output array
NS, MS = (1, 63, 64, 65, 257, 1499), (1, 2, 3, 16, 17, 33, 64)


class Buffers:
    """sums [T_out, 5], reliability [T_out, n_thr, M + 1, 2] and cell_crps [n] (``carried`` or
    zeros), each inside a canary-filled allocation; only the names of ``want`` are handed over."""

    def __init__(self, n, M, n_thr, T_out, dev, want=sc.NAMES, carried=None):
        shapes = {"sums": (T_out, 5), "reliability": (T_out, n_thr, M + 1, 2), "cell_crps": (n,)}
        self.full, self.view, self.want = {}, {}, tuple(want)
        for k, shape in shapes.items():
            size = int(np.prod(shape))
            if k == "reliability":
                self.full[k] = torch.full((size + 2 * PAD,), int(sc.CANARY_L), device=dev, dtype=torch.int64)
            else:
                self.full[k] = torch.full((size + 2 * PAD,), float(sc.CANARY_D), device=dev, dtype=torch.float64)
            self.view[k] = self.full[k][PAD:PAD + size].view(shape)
        self.carried = np.zeros(n) if carried is None else np.asarray(carried, np.float64)
        self.view["cell_crps"].copy_(torch.from_numpy(self.carried))

    def pointers(self):
        return {k: self.view[k].data_ptr() for k in self.want if self.view[k].numel()}

    def pads_intact(self):
        for k, b in self.full.items():
            c = int(sc.CANARY_L) if k == "reliability" else float(sc.CANARY_D)
            if not (bool((b[:PAD] == c).all()) and bool((b[-PAD:] == c).all())):
                return False
        return True

    def check(self, ref, label=""):
        """The pads hold their canaries; every array handed over equals ``ref`` (which holds the
        canary in the columns the call must not touch), every other array is as it was."""
        assert self.pads_intact(), f"{label}: canary overwritten"
        for k in sc.NAMES:
            got = self.view[k].cpu().numpy()
            if k in self.want:
                w = ref[k]
            elif k == "cell_crps":
                w = self.carried
            else:
                w = np.full(got.shape, sc.CANARY_L if k == "reliability" else sc.CANARY_D, got.dtype)
            assert got.dtype == w.dtype and got.shape == w.shape, f"{label}: {k}"
            assert np.array_equal(got, w, equal_nan=got.dtype.kind == "f"), f"{label}: {k}"

    def untouched(self):
        ref = {"sums": np.full(self.view["sums"].shape, sc.CANARY_D), "cell_crps": self.carried,
               "reliability": np.full(self.view["reliability"].shape, sc.CANARY_L)}
        return self.pads_intact() and all(np.array_equal(self.view[k].cpu().numpy(), ref[k]) for k in sc.NAMES)


def scores_update(pred, row0, n, truth, truth_row0, t_truth0, thr, bufs, t_begin, t_count, T_out, t_out0, stream=None,
                  M=None, n_thr=None, T=None, Tt=None):
    th = (C.c_float * 8)(*thr)
    o = _lib.MswEnsembleScoresOut(**bufs.pointers())
    r = (C.c_int64 * 65)(*[int(v) for v in row0])
    st = C.c_void_p(stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    return _lib.lib().msw_ensemble_scores_update(
        C.c_void_p(pred.data_ptr()), pred.shape[2] if T is None else T, t_begin, t_count, r,
        len(row0) if M is None else M, n, C.c_void_p(truth.data_ptr()), truth.shape[2] if Tt is None else Tt, t_truth0,
        int(truth_row0), th, len(thr) if n_thr is None else n_thr, T_out, t_out0, C.byref(o), st)


def on_device(host, cuda):
    return torch.from_numpy(np.ascontiguousarray(host)).to(cuda)


def run(host, dev, row0, n, truth, dtruth, truth_row0, t_truth0, thr, t_begin=0, t_count=None, T_out=None, t_out0=0,
        want=sc.NAMES, carried=None, label=""):
    """One raw ABI call into canary buffers, checked against the restatement."""
    t_count = host.shape[2] - t_begin if t_count is None else t_count
    T_out = t_count if T_out is None else T_out
    bufs = Buffers(n, len(row0), len(thr), T_out, dev.device, want, carried)
    _lib.check(scores_update(dev, row0, n, dtruth, truth_row0, t_truth0, thr, bufs, t_begin, t_count, T_out, t_out0))
    bufs.check(sc.scores_reference(host, row0, n, truth, truth_row0, t_truth0, thr, t_begin, t_count, T_out, t_out0,
                                   carried), label)
    return bufs


def run_case(c, cuda, label="", **kw):
    dev = on_device(c["pred"], cuda)
    dtruth = dev if c["truth"] is c["pred"] else on_device(c["truth"], cuda)
    return run(c["pred"], dev, c["row0"], c["n"], c["truth"], dtruth, c["truth_row0"], c["t_truth0"], c["thr"],
               carried=c["carried"], label=label, **{**c["window"], **kw})


# ------------------------------------------------------------------ 1. shape sweep
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("T", [1, 47, 48, 65])
def test_shape_sweep(cuda, T, M):
    """Every (n, M, T): the whole window, all outputs, four thresholds, the truth in an array of
    its own; and one of five further variants -- the truth as one more range of pred; an
    unaligned window without thresholds into a truth with its own stride and offset; each output
    alone; a carried cell_crps and columns t_out0 > 0 of a wider output; three thresholds in
    windows of 1, 16 and 17 steps."""
    for i_n, n in enumerate(NS):
        label = f"n={n} M={M} T={T}"
        seed = T + n + M
        h = ec.make_members(n, M, T, seed)
        y = sc.make_truth(h, seed)
        sc.assert_exact(h, y)
        host, row0 = ec.place(h, n + M)
        truth, trow0 = sc.place_truth(y, seed, T + 6, 3)
        dev, dtruth = on_device(host, cuda), on_device(truth, cuda)
        run(host, dev, row0, n, truth, dtruth, trow0, 3, sc.THR4, label=label)
        variant = (i_n + MS.index(M)) % 5
        if variant == 0:
            both, rows = ec.place(np.concatenate([h, y[None]]), seed)
            d = on_device(both, cuda)
            run(both, d, rows[:M], n, both, d, rows[M], 0, sc.THR4[:2], label=label + " aliased")
        elif variant == 1:
            tb = min(3, T - 1)
            tc = max((T - tb) // 2 * 2 - 1, 1)
            tr, r0 = sc.place_truth(y[:, tb:tb + tc], seed, tc + 11, 5)
            run(host, dev, row0, n, tr, on_device(tr, cuda), r0, 5, (), tb, tc, tc + 4, 3, label=label + f" window=({tb}, {tc})")
        elif variant == 2:
            for k in sc.NAMES:
                run(host, dev, row0, n, truth, dtruth, trow0, 3, sc.THR4[:2], want=(k,), label=label + " " + k)
        elif variant == 3:
            run(host, dev, row0, n, truth, dtruth, trow0, 3, sc.THR4[:1], 0, T, T + 9, 5,
                carried=sc.carried_values(n, seed), label=label + " carried")
        else:
            whole = sc.scores_reference(host, row0, n, truth, trow0, 3, sc.THR4[:3])
            for step in (1, 16, 17):
                bufs = Buffers(n, M, 3, T, cuda)
                for t0 in range(0, T, step):
                    _lib.check(scores_update(dev, row0, n, dtruth, trow0, 3 + t0, sc.THR4[:3], bufs, t0,
                                             min(step, T - t0), T, t0))
                bufs.check(whole, label + f" windows of {step}")


@pytest.mark.parametrize("name", list(sc.GRID_CASES))
def test_named_cases(cuda, name):
    run_case(sc.build_case(sc.CASES[name]), cuda, name)


def test_duplicate_member_and_repeat(cuda):
    """A range may repeat (that member counts twice), and two calls give the same bits."""
    h = ec.make_members(65, 3, 48, seed=7)
    y = sc.make_truth(h, 7)
    host, row0 = ec.place(h, seed=7)
    truth, trow0 = sc.place_truth(y, 7)
    row0 = np.array([row0[2], row0[0], row0[2], row0[1]])
    dev, dtruth = on_device(host, cuda), on_device(truth, cuda)
    for _ in range(2):
        run(host, dev, row0, 65, truth, dtruth, trow0, 0, sc.THR4)


# ------------------------------------------------------------------ 2. the cell loop
@pytest.mark.parametrize("rounds", [2, 3])
def test_several_rounds_per_workgroup(cuda, rounds):
    """Blocks long enough for two and three rounds of 32 cells at T = 2, the last block ragged."""
    M, T = 1, 2
    n = sc.cells_for_rounds(scores_launch, M, T, rounds)
    grid, per_round, iters = scores_launch(n, M, T)
    assert iters == rounds and per_round == 32 and grid * per_round * (iters - 1) < n <= grid * per_round * iters
    h = ec.make_members(n, M, T, seed=rounds)
    y = sc.make_truth(h, rounds)
    sc.assert_exact(h, y)
    host, row0 = ec.place(h, seed=rounds)
    truth, trow0 = sc.place_truth(y, rounds)
    assert host.nbytes < 32 << 20
    run(host, on_device(host, cuda), row0, n, truth, on_device(truth, cuda), trow0, 0, sc.THR4[:2],
        label=f"n={n} grid={grid} iters={iters}")


# ------------------------------------------------------------------ 3. full-precision data
@pytest.fixture(scope="module")
def full_case():
    return sc.build_case(sc.CASES["full_m7"])


def call_full(c, cuda, chunk):
    """The full-precision case scored in windows of ``chunk`` steps -> the three outputs (numpy)."""
    dev, dtruth = on_device(c["pred"], cuda), on_device(c["truth"], cuda)
    T = c["T"]
    bufs = Buffers(c["n"], c["M"], len(c["thr"]), T, cuda)
    for t0 in range(0, T, chunk):
        _lib.check(scores_update(dev, c["row0"], c["n"], dtruth, c["truth_row0"], t0, c["thr"], bufs, t0,
                                 min(chunk, T - t0), T, t0))
    assert bufs.pads_intact()
    return {k: bufs.view[k].cpu().numpy() for k in sc.NAMES}


def test_full_precision_within_the_bound(cuda, full_case):
    """Measured on an MI355X (profiles/ensemble/scores_bound_share.json): the largest
    |difference| / bound was 7.8e-5 (sum e^2) and 5.4e-5 (sum v); sum a, sum b, sum |e| and
    cell_crps equalled the restatement -- float32 depths in [0, 1.5] differ and add without
    rounding in float64 at this size, only the products round."""
    c = full_case
    got = call_full(c, cuda, c["T"])
    want = sc.reference_of(c)
    bound = sc.sum_bounds(c["h"], c["y"])
    share = np.abs(got["sums"] - want["sums"]) / bound
    cell_share = np.abs(got["cell_crps"] - want["cell_crps"]) / np.maximum(sc.cell_bound(c["h"], c["y"]), 1e-300)
    print("share of the bound per sum", dict(zip(sc.SUM_NAMES, share.max(0))), "cell_crps", cell_share.max())
    assert (share <= 1).all() and (cell_share <= 1).all()
    assert np.array_equal(got["reliability"], want["reliability"])


def test_chunked_equals_whole_bitwise_on_full_precision(cuda, full_case):
    whole = call_full(full_case, cuda, 48)
    for chunk in (1, 5, 16):
        assert sc.same(call_full(full_case, cuda, chunk), whole), chunk


# ------------------------------------------------------------------ 4. NaN
def test_planted_nan(cuda):
    c = sc.build_case(sc.CASES["m3"])
    pred = c["pred"].copy()
    pred[c["row0"][1] + 7, 0, 2] = np.nan          # a member: cell 7, step 2
    pred[c["truth_row0"] + 11, 0, 4] = np.nan      # the truth: cell 11, step 4
    dev = on_device(pred, cuda)
    bufs = run(pred, dev, c["row0"], c["n"], pred, dev, c["truth_row0"], 0, c["thr"])
    sums, cell = bufs.view["sums"].cpu().numpy(), bufs.view["cell_crps"].cpu().numpy()
    assert np.isnan(sums[[2, 4]]).all() and not np.isnan(sums[[0, 1, 3]]).any()
    assert list(np.nonzero(np.isnan(cell))[0]) == [7, 11]
    assert (bufs.view["reliability"].cpu().numpy()[..., 0].sum(2) == c["n"]).all()


# ------------------------------------------------------------------ 5. refusals leave the outputs alone
def test_abi_refusals_keep_the_canaries(cuda):
    n, M, T = 5, 3, 8
    h = ec.make_members(n, M, T, seed=1)
    host, row0 = ec.place(h, seed=1)
    truth, trow0 = sc.place_truth(sc.make_truth(h, 1), 1)
    dev, dtruth = on_device(host, cuda), on_device(truth, cuda)
    thr = sc.THR4[:2]
    bufs = Buffers(n, M, 2, T, cuda)
    ok = dict(pred=dev, row0=row0, n=n, truth=dtruth, truth_row0=trow0, t_truth0=0, thr=thr, bufs=bufs, t_begin=0,
              t_count=T, T_out=T, t_out0=0)
    bad = [dict(M=65), dict(M=0), dict(t_begin=-1), dict(t_begin=4, t_count=5), dict(t_count=-1), dict(t_out0=-1),
           dict(t_out0=1), dict(T_out=7), dict(n=-1), dict(row0=np.array([0, -1, 3])), dict(thr=sc.THR4 + (2.0,)),
           dict(n_thr=-1), dict(T=-1), dict(truth_row0=-1), dict(t_truth0=-1), dict(t_truth0=1), dict(Tt=7)]
    for kw in bad:
        assert scores_update(**{**ok, **kw}) == -1, kw      # MSW_ERR_INVALID
        assert bufs.untouched(), kw
    for kw in (dict(t_count=0), dict(n=0)):                 # no-ops
        assert scores_update(**{**ok, **kw}) == _lib.MSW_OK and bufs.untouched()
    none = Buffers(n, M, 2, T, cuda, want=())
    assert scores_update(**{**ok, "bufs": none}) == _lib.MSW_OK and none.untouched()
    _lib.check(scores_update(**ok))                         # and the good call still works
    bufs.check(sc.scores_reference(host, row0, n, truth, trow0, 0, thr))


# ------------------------------------------------------------------ 6. the wrapper and the engine
def test_wrapper_makes_no_synchronisation(cuda):
    c = sc.build_case(sc.CASES["tail"])
    pred, truth = on_device(c["pred"], cuda), on_device(c["truth"], cuda)
    ranges = [(int(r), int(r) + c["n"]) for r in c["row0"]]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        es = EnsembleScores(ranges, c["T"], c["thr"], device=cuda)
        for t0 in range(0, c["T"], 3):
            es.update(pred, truth, t0, min(3, c["T"] - t0), truth_row0=c["truth_row0"])
        res = es.result()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    want = sc.scores_reference(c["pred"], c["row0"], c["n"], c["truth"], c["truth_row0"], 0, c["thr"])
    assert np.array_equal(res["sums"].cpu().numpy(), want["sums"])
    assert np.array_equal(es.arrays["reliability"].cpu().numpy(), want["reliability"])
    assert np.array_equal(es.arrays["cell_crps"].cpu().numpy(), want["cell_crps"])
    cpu = ensemble_scores(torch.from_numpy(c["pred"]), torch.from_numpy(c["truth"]), ranges, c["thr"],
                          truth_row0=c["truth_row0"])
    for k in ("sums", "cell_crps"):                          # grid data: the torch path gives the same bits
        assert torch.equal(res[k].cpu(), cpu[k]), k
    for t in c["thr"]:
        assert _same(_to_cpu(res["reliability"][t]), cpu["reliability"][t]), t


@pytest.fixture(scope="module")
def engine(cuda):
    m = build_msgnn(4, 32, 4, state=weights("K4_F32")).to(cuda)
    m.engine = "hip"
    return m


@pytest.fixture(scope="module")
def ensemble(cuda):
    g = make_multiscale_mesh(**mesh_config("small"), T=48)
    bcs = [hydrograph_bc(48, peak=p, seed=s) for p, s in ((1.0, 1), (3.0, 2), (4.5, 3), (7.0, 4))]
    return make_ensemble(g, bcs).to(cuda)


def _to_cpu(u):
    if isinstance(u, dict):
        return {k: _to_cpu(v) for k, v in u.items()}
    return u.cpu() if isinstance(u, torch.Tensor) else u


def _same(u, v):
    if isinstance(u, dict):
        return u.keys() == v.keys() and all(_same(u[k], v[k]) for k in u)
    if not isinstance(u, torch.Tensor):
        return u == v
    return u.dtype == v.dtype and torch.equal(u, v)


def test_rollout_ensemble_with_truth(cuda, engine, ensemble):
    ranges = member_ranges(ensemble)
    plain, rollout = rollout_ensemble(engine, ensemble, 48, chunk=None, keep_rollout=True)
    assert set(plain) == {"maps", "steps"}
    control = ranges[3]                                       # the fourth run as the truth
    truth = rollout[control[0]:control[1]].clone()
    want = ensemble_scores(rollout, truth, ranges)
    for chunk in (16, None):
        out, kept = rollout_ensemble(engine, ensemble, 48, chunk=chunk, keep_rollout=True, truth=truth)
        assert torch.equal(kept, rollout) and _same(out["scores"], want), chunk
        assert _same(out["maps"], plain["maps"]) and _same(out["steps"], plain["steps"])
    rows = rollout_ensemble(engine, ensemble, 48, chunk=16, truth=rollout, truth_row0=control[0])
    assert _same(rows["scores"], want)
    s = want
    assert s["steps"] == 48 and s["members"] == 4 and bool((s["spread"] > 0).any()) and bool((s["crps"] > 0).any())
    n = control[1] - control[0]
    host = rollout.cpu().numpy()
    ref = sc.scores_reference(host, [r for r, _ in ranges], n, host, control[0], 0, (0.05, 0.3))
    bound = sc.sum_bounds(ec.gather(host, [r for r, _ in ranges], n), host[control[0]:control[1], 0])
    assert (np.abs(s["sums"].cpu().numpy() - ref["sums"]) <= bound).all()
    assert np.array_equal(s["reliability"][0.05]["n"].cpu().numpy(), ref["reliability"][:, 0, :, 0])
    assert np.array_equal(s["reliability"][0.3]["observed"].cpu().numpy(), ref["reliability"][:, 1, :, 1])


def test_update_behind_rollout_on_a_side_stream(cuda, engine, ensemble):
    from mswegnn.engine import plan_for
    ranges = member_ranges(ensemble)
    whole = engine.rollout(ensemble, 48)
    want = ensemble_scores(whole, whole, ranges[:3], truth_row0=ranges[3][0])
    plan = plan_for(engine, ensemble)
    side = torch.cuda.Stream(cuda)
    es = EnsembleScores(ranges[:3], 48, device=cuda)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = plan.rollout(ensemble.x, ensemble.BC, ensemble.node_BC, ensemble.type_BC, 48)
        es.update(out, out, truth_row0=ranges[3][0])   # enqueued directly behind the rollout
        res = es.result()
    side.synchronize()
    assert torch.equal(out, whole) and _same(res, want)
