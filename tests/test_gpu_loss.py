"""The training-loss kernels (msw_train_loss_forward / _backward, csrc/loss.hip) and their wrapper
(mswegnn.loss.loss_function) on the GPU against the numpy restatement of tests/loss_cases.py: the
record bit for bit on grid data (every sum exact in fp64 in any order), within the derived
2 n 2^-53 sum|term| on full-precision data; the gradients bit for bit from the kernel's own
record, and within one fp32 ulp of torch's float64 autograd of oracle/loss_ref.py.  Every output
sits between canaries.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import loss_cases as lc
import loss_ref  # oracle/
from conftest import build_msgnn, golden, rel_err, weights
from test_loss import FX_BOUND

pytestmark = pytest.mark.gpu

PAD = 64
CANARY = -123456.0


def _launch(total):
    from mswegnn.loss import launch
    return launch(total)


class _Guarded:
    """An output buffer of `shape` between two pads of canaries."""

    def __init__(self, shape, dtype, dev):
        n = int(np.prod(shape)) if len(shape) else 1
        self.buf = torch.full((n + 2 * PAD,), CANARY, dtype=dtype, device=dev)
        self.view = self.buf[PAD:PAD + n]
        self.shape = shape

    def ptr(self):
        return self.view.data_ptr()

    def get(self):
        b = self.buf.cpu()
        assert (b[:PAD] == CANARY).all() and (b[-PAD:] == CANARY).all(), "an output's canaries were overwritten"
        return b[PAD:-PAD].reshape(self.shape).numpy().copy()


def run_abi(dev, case, tl, mask, vs, g=1.0, cons=None, want_gin=True):
    """Forward and backward through the C ABI -> (record, loss, grad_pred, grad_input_h or None)."""
    from mswegnn import _lib as L
    from mswegnn.loss import make_desc, workspace
    cons = case["cons"] if cons is None else cons
    n = case["pred"].shape[0]
    pred, real = torch.from_numpy(case["pred"]).to(dev), torch.from_numpy(case["real"]).to(dev)
    keep, kw = [], {}
    if cons:
        t = {k: torch.from_numpy(np.ascontiguousarray(cons[k])).to(dev) for k in ("area", "input_h", "node_bc", "bc", "length")}
        keep.append(t)
        kw = dict(conservation=cons["c"], num_graphs=cons["num_graphs"], seconds_per_step=cons["seconds"],
                  area=t["area"].data_ptr(), input_h=t["input_h"].data_ptr(), input_h_stride=1,
                  node_bc=t["node_bc"].data_ptr(), bc=t["bc"].data_ptr(), edge_bc_length=t["length"].data_ptr(),
                  n_bc=int(t["node_bc"].numel()))
    d = make_desc(n, case["ranges"], tl, mask, vs, **kw)
    scratch = _Guarded((workspace(d),), torch.float64, dev)
    rec, loss = _Guarded((L.TRAIN_LOSS_RECORD,), torch.float64, dev), _Guarded((), torch.float32, dev)
    gp = _Guarded((n, 2), torch.float32, dev)
    gin = _Guarded((n,), torch.float32, dev) if cons and want_gin else None
    gout = torch.tensor(g, dtype=torch.float32, device=dev)
    lib = L.lib()
    L.check(lib.msw_train_loss_forward(C.byref(d), pred.data_ptr(), real.data_ptr(), scratch.ptr(), loss.ptr(), rec.ptr(),
                                       None))
    L.check(lib.msw_train_loss_backward(C.byref(d), pred.data_ptr(), real.data_ptr(), rec.ptr(), gout.data_ptr(),
                                        gp.ptr(), gin.ptr() if gin is not None else None, None))
    torch.cuda.synchronize()
    scratch.get()
    return rec.get(), loss.get(), gp.get(), gin.get() if gin is not None else None


def check_case(dev, case, tl, mask, vs, g=1.0, clean=None):
    """One case against the restatement (of `clean`, the same case before rows outside the ranges
    were poisoned) -> (record, grad_pred, grad_input_h)."""
    ref = clean or case
    cons = ref["cons"]
    rec, loss, gp, gin = run_abi(dev, case, tl, mask, vs, g)
    want = lc.restate(ref["pred"], ref["real"], ref["ranges"], tl, mask, vs, **cons)
    label = (tl, mask, vs, case["ranges"][:3])
    if case["full"]:
        b = lc.bound(ref["pred"], ref["real"], ref["ranges"], tl, mask, **cons)
        assert (np.abs(rec[:4] - want[:4]) <= b).all(), (label, rec[:4], want[:4], b)
        assert rec[lc.N] == want[lc.N]
        rl = abs(rec[lc.LOSS] - want[lc.LOSS]) / abs(want[lc.LOSS])
        assert rl <= 1e-12, (label, rl)
    else:
        assert lc.same_bits(rec, want), (label, rec, want)
    assert lc.same_bits(loss, np.float32(rec[lc.LOSS])), label
    c = cons.get("c", 0.0)
    wgp, wgin = lc.gradient(ref["pred"], ref["real"], ref["ranges"], rec, g, tl, mask, c, cons.get("area"),
                            cons.get("node_bc"))
    assert lc.same_bits(gp, wgp), label
    if gin is not None:
        assert lc.same_bits(gin, wgin), label
    return rec, gp, gin


def _ulp_of_float64_autograd(case, tl, mask, vs, gp, g=1.0):
    """grad_pred within one fp32 ulp of torch float64 autograd of oracle/loss_ref.py, NaN for NaN."""
    p = torch.from_numpy(case["pred"]).double().requires_grad_(True)
    data = lc_graph(case["ranges"])
    loss = loss_ref.loss_function(p, torch.from_numpy(case["real"]).double(), data, type_loss=tl, only_where_water=mask,
                                  velocity_scaler=vs)
    (loss * g).backward()
    g64 = p.grad.numpy()
    nan = np.isnan(g64)
    assert np.array_equal(np.isnan(gp), nan)
    ulp = np.spacing(np.abs(g64).astype(np.float32)).astype(np.float64)
    assert (np.abs(gp.astype(np.float64) - g64)[~nan] <= ulp[~nan]).all()
    assert (gp[g64 == 0] == 0).all()
    return float(loss.detach())


def lc_graph(ranges):
    from mswegnn.mesh import Graph
    return Graph(node_ptr=torch.tensor([[s, e] for s, e in ranges]))


@pytest.mark.parametrize("rows", [1, 255, 256, 257, 1499])
def test_sweep_rows_starts_and_options(cuda, rows):
    """Row counts {1, 255, 256, 257, 1499} x range starts {0, 5} x RMSE / MAE x mask x
    velocity_scaler {1, 7} on grid data: record bit-equal, loss = float32(record.loss), gradients
    bit-equal from that record and within 1 fp32 ulp of float64 autograd, zeros outside the range."""
    for start in (0, 5):
        case = lc.build_case(dict(sizes=[rows], gaps=[start], seed=100 + rows + start), _launch)
        for tl, mask, vs in lc.OPTIONS:
            rec, gp, _ = check_case(cuda, case, tl, mask, vs)
            want = _ulp_of_float64_autograd(case, tl, mask, vs, gp)
            if not np.isnan(want):
                assert abs(rec[lc.LOSS] - want) <= 1e-14 * abs(want)


@pytest.mark.parametrize("name", ["full_1499", "full_cons"])
def test_full_precision_data_within_the_derived_bound(cuda, name):
    case = lc.build_case(lc.CASES[name], _launch)
    for tl, mask, vs in lc.OPTIONS:
        check_case(cuda, case, tl, mask, vs, g=0.25)


@pytest.mark.parametrize("name", ["two_iterations", "three_iterations"])
def test_row_loop_rounds(cuda, name):
    """Two and three rounds of the grid-stride loop (row counts from msw_train_loss_launch), the last
    round ragged: bit-equal on grid data."""
    case = lc.build_case(lc.CASES[name], _launch)
    total = sum(e - s for s, e in case["ranges"])
    grid, per, iters = _launch(total)
    assert iters == lc.CASES[name]["iters"] and grid * per * (iters - 1) < total
    for tl, mask, vs in (("RMSE", True, 7.0), ("MAE", False, 1.0)):
        check_case(cuda, case, tl, mask, vs)


@pytest.mark.parametrize("name", ["empty_first", "empty_middle", "empty_last", "five_sims", "row0_5", "cons_batch3"])
@pytest.mark.parametrize("value", [7e8, float("nan")])
def test_ranges_and_poisoned_rows_outside(cuda, name, value):
    """1 - 5 ranges with an empty one in each position; rows outside every range hold 7e8 / NaN in
    preds and real: the loss is that of the clean data and their gradient is exactly +0 (a ghost
    cell outside the ranges keeps its values: the correction reads it)."""
    clean = lc.build_case(lc.CASES[name], _launch)
    case = dict(clean)
    case["pred"], case["real"] = lc.poison([clean["pred"], clean["real"]], clean["ranges"], value)
    if clean["cons"]:
        # the ghost cell outside the ranges is read by the correction: it keeps its values
        nb = [int(k) for k in clean["cons"]["node_bc"]]
        for k in nb:
            case["pred"][k], case["real"][k] = clean["pred"][k], clean["real"][k]
    inside = np.zeros(clean["num_rows"], bool)
    for s, e in clean["ranges"]:
        inside[s:e] = True
    for tl, mask, vs in (("RMSE", True, 7.0), ("MAE", True, 1.0), ("RMSE", False, 1.0)):
        rec, gp, gin = check_case(cuda, case, tl, mask, vs, clean=clean)
        assert np.isfinite(rec[lc.LOSS])
        out = ~inside
        if clean["cons"]:
            out[[int(k) for k in clean["cons"]["node_bc"]]] = False
        assert lc.same_bits(gp[out], np.zeros_like(gp[out]))


def _special(rows, edit):
    case = lc.build_case(dict(sizes=[rows], gaps=[3], seed=77), _launch)
    edit(case)
    return case


def test_semantics_table(cuda):
    """The degenerate and special-value rows of the issue's table, NaN positions compared exactly
    (same_bits), against the restatement and against float64 autograd of oracle/loss_ref.py."""
    s, e = 3, 3 + 300

    def all_equal(c):
        c["pred"][:] = c["real"]
    case = _special(300, all_equal)
    for tl in ("RMSE", "MAE"):   # no selected row: loss NaN, every gradient 0
        rec, gp, _ = check_case(cuda, case, tl, True, 7.0)
        assert rec[lc.N] == 0 and np.isnan(rec[lc.LOSS]) and lc.same_bits(gp, np.zeros_like(gp))
    # the same data without the mask: RMSE S = 0, n > 0 -> loss 0, gradients NaN (0 * inf) in the range
    rec, gp, _ = check_case(cuda, case, "RMSE", False, 7.0)
    assert rec[lc.LOSS] == 0 and np.isnan(gp[s:e]).all() and lc.same_bits(gp[:s], np.zeros_like(gp[:s]))
    _ulp_of_float64_autograd(case, "RMSE", False, 7.0, gp)
    rec, gp, _ = check_case(cuda, case, "MAE", False, 7.0)   # MAE, d = 0: gradient 0
    assert rec[lc.LOSS] == 0 and lc.same_bits(gp, np.zeros_like(gp))

    def only_h(c):
        c["pred"][:, 1] = c["real"][:, 1]
    case = _special(300, only_h)   # RMSE column v: S_v = 0, n > 0
    for mask in (False, True):
        rec, gp, _ = check_case(cuda, case, "RMSE", mask, 7.0)
        d = case["pred"][s:e, 0] != case["real"][s:e, 0]
        sel = d if mask else np.ones_like(d)
        assert np.isfinite(rec[lc.LOSS]) and rec[lc.SV] == 0 and rec[lc.N] == sel.sum()
        assert np.isnan(gp[s:e, 1][sel]).all() and np.isfinite(gp[s:e, 0]).all()
        assert lc.same_bits(gp[s:e][~sel], np.zeros_like(gp[s:e][~sel]))
        _ulp_of_float64_autograd(case, "RMSE", mask, 7.0, gp)

    def minus_zero(c):
        c["pred"][:] = c["real"]
        c["pred"][:, 0], c["real"][:, 0] = 0.0, -0.0
        c["pred"][10, 1] = c["real"][10, 1] + np.float32(0.5)
    case = _special(300, minus_zero)   # 0 - (-0.0): not water; one wet row
    rec, gp, _ = check_case(cuda, case, "MAE", True, 1.0)
    assert rec[lc.N] == 1 and np.count_nonzero(gp) == 1

    # NaN / inf in a range row: the row is selected and the loss is NaN (an inf against a finite
    # target gives an inf loss, as in torch; inf - inf is the NaN case)
    for bad in (np.float32("nan"), np.float32("inf")):
        def special(c, bad=bad):
            c["pred"][20, 0] = bad
        case = _special(300, special)
        for tl in ("RMSE", "MAE"):
            rec, gp, _ = check_case(cuda, case, tl, True, 7.0)
            clean = lc.build_case(dict(sizes=[300], gaps=[3], seed=77), _launch)
            n_clean = lc.restate(clean["pred"], clean["real"], clean["ranges"], tl, True, 7.0)[lc.N]
            d20 = (clean["pred"][20] != clean["real"][20]).any()
            assert rec[lc.N] == n_clean + (0 if d20 else 1)
            assert np.isnan(rec[lc.LOSS]) if np.isnan(bad) else np.isinf(rec[lc.LOSS])


def test_conservation_sign_and_input_gradient(cuda):
    """cons > 0, < 0 and == 0 through the ABI on grid data (record and gradients bit-equal);
    grad_input_h is the exact negative of the conservation part of grad_pred's h column; without
    the grad_input_h output grad_pred is the same."""
    seen = set()
    base = lc.build_case(lc.CASES["cons_batch3"], _launch)
    for variant in ("as_is", "rising_without_inflow", "balanced"):
        case = dict(base, cons=dict(base["cons"]))
        if variant == "rising_without_inflow":   # every cell 8 m deeper, nothing flows in: cons > 0
            case["cons"]["input_h"] = case["pred"][:, 0] - np.float32(8)
            case["cons"]["bc"] = np.zeros_like(case["cons"]["bc"])
        if variant == "balanced":   # no volume change, no inflow: cons = 0 and its gradient 0
            case["cons"]["input_h"] = case["pred"][:, 0].copy()
            case["cons"]["bc"] = np.zeros_like(case["cons"]["bc"])
        for tl, mask in (("RMSE", True), ("MAE", False)):
            rec, gp, gin = check_case(cuda, case, tl, mask, 7.0, g=0.25)
            seen.add(float(np.sign(rec[lc.CONS])))
            rec0, _, gp0, _ = run_abi(cuda, case, tl, mask, 7.0, 0.25, cons={})
            _, _, gp_no_gin, _ = run_abi(cuda, case, tl, mask, 7.0, 0.25, want_gin=False)
            assert lc.same_bits(gp, gp_no_gin)
            m = ((np.float64(np.float32(0.25)) * rec[lc.CC]) * case["cons"]["area"].astype(np.float64)).astype(np.float32)
            plain = np.ones(case["num_rows"], bool)
            plain[[int(k) for k in case["cons"]["node_bc"]]] = False
            inside = np.zeros(case["num_rows"], bool)
            for s, e in case["ranges"]:
                inside[s:e] = True
            rows = plain & inside
            assert lc.same_bits(gin[rows], -m[rows]) and lc.same_bits(gp[rows, 0], gp0[rows, 0] + m[rows])
            assert lc.same_bits(gp[:, 1], gp0[:, 1])
            if variant == "balanced":
                assert rec[lc.CONS] == 0 and rec[lc.CC] == 0 and lc.same_bits(gp, gp0)
                assert not gin.any()
    assert seen == {1.0, -1.0, 0.0}


def _wrapper_case(dev, fx, key, g=1.0):
    from mswegnn.loss import loss_function
    case = lc.fixture_case(fx, key)
    preds = torch.from_numpy(case["pred"]).to(dev).requires_grad_(True)
    data, BC = lc.fixture_data(fx, case["layout"], case["x_h"], device=dev, preds=preds if case["alias"] else None)
    loss = loss_function(preds, torch.from_numpy(case["real"]).to(dev), data, BC, type_loss=case["type_loss"],
                         only_where_water=case["mask"], conservation=case["cons"].get("c", 0),
                         velocity_scaler=int(case["vs"]))
    (loss * g).backward()
    return case, loss.detach().cpu(), preds.grad.cpu()


def test_wrapper_against_the_reference_fixture(cuda):
    """mswegnn.loss.loss_function on the GPU on every case of fx_loss.npz (the reference's own
    loss_function and autograd: Data, Batch, single scale; the conservation term with cons > 0 and
    < 0; data.x aliasing preds): loss and gradient within FX_BOUND (twice the reference's own fp32
    distance from the float64 restatement, tests/test_loss.py)."""
    from mswegnn.loss import LOSS_CALLS
    fx = golden("fx_loss")
    calls = LOSS_CALLS[0]
    for key in fx["cases"]:
        case, loss, grad = _wrapper_case(cuda, fx, str(key))
        assert loss.dtype == torch.float32 and grad.dtype == torch.float32
        el = abs(float(loss) - float(case["loss"])) / abs(float(case["loss"]))
        eg = rel_err(grad, case["grad"])
        assert el <= FX_BOUND and eg <= FX_BOUND, (key, el, eg)
    assert LOSS_CALLS[0] == calls + len(fx["cases"])


def test_aliased_input_depth_gives_zero_net_conservation_gradient(cuda):
    """training_step feeds the prediction back before the loss, so data.x[:, -2] is preds[:, 0]
    through another autograd path: delta_WD is 0, the volume and the correction vanish, and the two
    conservation gradients cancel in every row -- the net gradient is the data term's to within the
    rounding of the conservation part (exactly, where the data term is 0)."""
    from mswegnn.loss import loss_function
    fx = golden("fx_loss")
    case = lc.fixture_case(fx, "batch/alias")
    real = torch.from_numpy(case["real"]).to(cuda)
    grads = {}
    for c in (0.0, 0.5):
        preds = torch.from_numpy(case["pred"]).to(cuda).requires_grad_(True)
        data, BC = lc.fixture_data(fx, "batch", case["x_h"], device=cuda, preds=preds)
        loss_function(preds, real, data, BC, "RMSE", True, c, 7).backward()
        grads[c] = preds.grad.cpu().numpy()
    rec = lc.restate(case["pred"], case["real"], case["ranges"], "RMSE", True, 7.0, **case["cons"])
    assert rec[lc.VOL] == 0 and rec[lc.CORR] == 0 and rec[lc.CONS] < 0
    m = np.abs(rec[lc.CC] * case["cons"]["area"].astype(np.float64))
    diff = np.abs(grads[0.5][:, 0].astype(np.float64) - grads[0.0][:, 0])
    assert (diff <= 2.0 ** -23 * (m + np.abs(grads[0.0][:, 0]))).all()
    assert lc.same_bits(grads[0.5][:, 1], grads[0.0][:, 1])
    zero = grads[0.0][:, 0] == 0
    assert zero.any() and lc.same_bits(grads[0.5][zero, 0], grads[0.0][zero, 0])


def test_wrapper_grad_out_streams_and_reruns(cuda):
    """grad_out = 0.25 (training_step's mean over R = 4 steps) reaches the kernels from the device;
    a side stream behind an engine rollout gives the default stream's bits; two runs are
    bit-identical."""
    from mswegnn.loss import loss_function
    from mswegnn.mesh import make_multiscale_mesh, mesh_config
    fx = golden("fx_loss")
    key = "batch/RMSE_m1_v7_c0.5"
    case, loss, grad = _wrapper_case(cuda, fx, key, g=0.25)
    rec = lc.restate(case["pred"], case["real"], case["ranges"], "RMSE", True, 7.0, **case["cons"])
    want, _ = lc.gradient(case["pred"], case["real"], case["ranges"], rec, 0.25, "RMSE", True, 0.5,
                          case["cons"]["area"], case["cons"]["node_bc"])
    assert rel_err(grad, want) <= FX_BOUND
    _, loss2, grad2 = _wrapper_case(cuda, fx, key, g=0.25)
    assert lc.same_bits(loss.numpy(), loss2.numpy()) and lc.same_bits(grad.numpy(), grad2.numpy())

    g = make_multiscale_mesh(**mesh_config("small"), T=4).to(cuda)
    m = build_msgnn(4, 32, 4, state=weights("K4_F32")).to(cuda)
    real = g.y[:, :, 3].contiguous()
    BC = g.BC[:, -2:, 3].mean(1)
    g.edge_BC_length = g.edge_BC_length[:1]

    def step():
        r = m.rollout(g, 4)
        preds = r[:, :, 3].contiguous().requires_grad_(True)
        loss = loss_function(preds, real, g, BC, "RMSE", True, 0.5, 7)
        loss.backward()
        return loss.detach(), preds.grad
    l0, g0 = step()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        l1, g1 = step()
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.isfinite(l0) and lc.same_bits(l0.cpu().numpy(), l1.cpu().numpy())
    assert lc.same_bits(g0.cpu().numpy(), g1.cpu().numpy())


def test_wrapper_under_autocast_computes_in_fp32(cuda):
    """Under autocast (main.py trains with precision='16-mixed') half-precision predictions are
    cast to fp32 and the HIP kernels run: the loss is the fp32 call's on the same values bit for
    bit, and the gradient comes back in the predictions' dtype."""
    from mswegnn.loss import LOSS_CALLS, loss_function
    fx = golden("fx_loss")
    case = lc.fixture_case(fx, "batch/RMSE_m1_v7_c0.5")
    real = torch.from_numpy(case["real"]).to(cuda)
    half = torch.from_numpy(case["pred"]).to(cuda).half().requires_grad_(True)
    full = half.detach().float().requires_grad_(True)
    data, BC = lc.fixture_data(fx, "batch", case["x_h"], device=cuda)
    calls = LOSS_CALLS[0]
    with torch.autocast("cuda", dtype=torch.float16):
        l16 = loss_function(half, real, data, BC, "RMSE", True, 0.5, 7)
    l32 = loss_function(full, real, data, BC, "RMSE", True, 0.5, 7)
    assert LOSS_CALLS[0] == calls + 2 and l16.dtype == torch.float32
    l16.backward()
    l32.backward()
    assert lc.same_bits(l16.detach().cpu().numpy(), l32.detach().cpu().numpy())
    assert half.grad.dtype == torch.float16
    assert torch.equal(half.grad, full.grad.half())


def test_wrapper_does_not_synchronise_the_host(cuda):
    """Under torch.cuda.set_sync_debug_mode("error") the torch composition with the water mask
    raises (its boolean-mask index is a nonzero and a device-to-host read); the wrapper's forward
    and backward pass once ptr_list has read node_ptr and temporal_res."""
    from mswegnn.loss import loss_function, torch_loss_function
    fx = golden("fx_loss")
    case = lc.fixture_case(fx, "batch/RMSE_m1_v7_c0.5")
    real = torch.from_numpy(case["real"]).to(cuda)
    preds = torch.from_numpy(case["pred"]).to(cuda).requires_grad_(True)
    data, BC = lc.fixture_data(fx, "batch", case["x_h"], device=cuda)
    args = (preds, real, data, BC, "RMSE", True, 0.5, 7)
    loss_function(*args).backward()   # warm: ptr_list reads node_ptr / temporal_res once
    preds.grad = None
    gscale = torch.tensor(0.25, device=cuda)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch_loss_function(*args)
        loss = loss_function(*args)
        (loss * gscale).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(loss) and torch.isfinite(preds.grad).all()


@pytest.mark.parametrize("sname,R", [("b1", 1), ("b1", 4), ("b2", 1), ("b2", 4)])
def test_training_step_with_the_fused_loss(cuda, sname, R, monkeypatch):
    """oracle/loss_ref.py's training_step with the fused loss in place of its own, every layer on
    the HIP training kernels, on the small-mesh fixtures (one graph and a two-graph batch, R = 1
    and 4): the reference's loss and every parameter gradient (fx_grad_train_K4_F32) at the bar
    tests/test_gpu_train.py holds the same fixtures to (its TOL and grad_cases.check with the
    reference's fp32 noise); the HIP loss ran R times."""
    import grad_cases as gc
    import msgnn_torch as orc
    from mswegnn import loss as ml
    from test_gpu_train import TOL

    def fused(preds, real, data, **kw):
        return ml.loss_function(preds, real, data, None, **kw)
    monkeypatch.setattr(loss_ref, "loss_function", fused)
    calls = ml.LOSS_CALLS[0]
    ours, fx = gc.training_step_case(cuda, sname, R)
    assert ml.LOSS_CALLS[0] == calls + R
    pre = f"{sname}_R{R}__"
    names = gc.manifest()["fx_grad_train_K4_F32_sets"][sname]
    monkeypatch.undo()   # the noise ensemble is the reference's arithmetic, not ours
    noise = gc.reference_fp32_noise(lambda: gc.training_batch(f"{sname}__", names, 5, fx, torch.device("cpu")),
                                    gc.weights("K4_F32"), orc.msgnn_config(num_scales=4, hid_features=32, K=4),
                                    R, fx, f"{sname}_R{R}_fp64__", p32=pre)
    worst, rule64 = gc.check(ours, fx, pre, TOL, f"{sname}_R{R}_fp64__", noise=noise)
    print(f"fused-loss training_step {sname} R={R}: loss {float(ours['loss']):.7e} (reference "
          f"{float(fx[pre + 'loss']):.7e}), worst {worst:.2e}; fp64 rule for {rule64}")
