"""The training loss (mswegnn/loss.py, csrc/loss.hip) on the CPU: the numpy restatement of the
kernels (tests/loss_cases.py) against its yardsticks -- oracle/loss_ref.py in float64, torch float64
autograd, and the reference's own loss_function values and gradients in tests/golden/fx_loss.npz
(tools/gen_golden_loss.py) -- the module's torch composition against the same fixture, the wrong
variants each caught by a named case, the C ABI's host-only checks and the opt-in hook.  The kernels
themselves are held to the restatement in tests/test_gpu_loss.py.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import loss_cases as lc
import loss_ref  # oracle/
from conftest import PKG, ROOT, golden, rel_err
from mswegnn.mesh import Graph

# The largest relative distance (max|a - b| / max|b|, losses |a - b| / |b|) of the REFERENCE's own
# fp32 loss and gradients in fx_loss.npz from the float64 restatement, over all 49 cases, as
# test_fixture_distance_is_the_measured_one measures it again: 2.4e-07 (a loss; gradients 1.2e-07).
# The bound for fp32 results against the fixture off its CPU, and for the HIP kernels, is twice that.
MEASURED_REF_FP32 = 2.4e-07
FX_BOUND = 2 * MEASURED_REF_FP32


def _data_for(ranges):
    """loss_ref's view of the graph: node_ptr [G, 2] (the finest range of every graph)."""
    return Graph(node_ptr=torch.tensor([[s, e] for s, e in ranges]))


def _loss_ref64(case, tl, mask, vs):
    p = torch.from_numpy(case["pred"]).double().requires_grad_(True)
    r = torch.from_numpy(case["real"]).double()
    loss = loss_ref.loss_function(p, r, _data_for(case["ranges"]), type_loss=tl, only_where_water=mask,
                                  velocity_scaler=vs)
    loss.backward()
    return float(loss.detach()), p.grad.numpy()


@pytest.mark.parametrize("name", [n for n, s in lc.CASES.items() if not s.get("cons") and "iters" not in s])
def test_restatement_equals_loss_ref_float64(name):
    """The restatement's loss equals oracle/loss_ref.py run in float64 to 1e-14 relative, and its
    closed-form gradient is the fp32 rounding of torch's float64 autograd of it (half an fp32 ulp
    plus 1e-13), for every option set; rows outside the ranges get exactly 0."""
    case = lc.build_case(lc.CASES[name], lc.host_launch)
    for tl, mask, vs in lc.OPTIONS:
        rec = lc.restate(case["pred"], case["real"], case["ranges"], tl, mask, vs)
        want, g64 = _loss_ref64(case, tl, mask, vs)
        assert abs(rec[lc.LOSS] - want) <= 1e-14 * abs(want), (name, tl, mask, vs, rec[lc.LOSS], want)
        gp, _ = lc.gradient(case["pred"], case["real"], case["ranges"], rec, 1.0, tl, mask)
        nan = np.isnan(g64)   # 0 * inf where an RMSE column has S_c = 0: the same positions
        assert np.array_equal(np.isnan(gp), nan), (name, tl, mask, vs)
        tol = np.abs(g64) * (2.0 ** -24 + 1e-13) + 2.0 ** -150
        assert (np.abs(gp.astype(np.float64) - g64)[~nan] <= tol[~nan]).all(), (name, tl, mask, vs)
        assert (gp[g64 == 0] == 0).all()


def _fx():
    return golden("fx_loss")


def _same_cpu(fx):
    import test_oracle_golden as tog
    return str(fx["cpu"]) == tog._cpu_model()


def _distance(case, loss, grad):
    """(loss, gradient) relative distances of fp32 results from the float64 restatement."""
    rec = lc.restate(case["pred"], case["real"], case["ranges"], case["type_loss"], case["mask"], case["vs"],
                     **case["cons"])
    c = case["cons"].get("c", 0.0)
    gp, gin = lc.gradient(case["pred"], case["real"], case["ranges"], rec, 1.0, case["type_loss"], case["mask"], c,
                          case["cons"].get("area"), case["cons"].get("node_bc"))
    if case["alias"]:   # data.x[:, -2] is preds[:, 0]: both gradients arrive at preds
        gp = gp.copy()
        gp[:, 0] = gp[:, 0] + gin
    return abs(float(loss) - rec[lc.LOSS]) / abs(rec[lc.LOSS]), rel_err(grad, gp)


def test_fixture_distance_is_the_measured_one():
    """The reference's own fp32 values against the float64 restatement, every case of fx_loss.npz:
    the distance this file's bound is derived from (MEASURED_REF_FP32 = 2.4e-07; the bound is twice
    it).  The conservation cases pin the term oracle/loss_ref.py lacks: cons > 0 (RMSE cases) and
    cons < 0 (MAE cases) both occur, and the aliased case's gradient is the sum of both paths."""
    fx = _fx()
    worst_l = worst_g = 0.0
    signs = set()
    for key in fx["cases"]:
        case = lc.fixture_case(fx, str(key))
        e_l, e_g = _distance(case, case["loss"], case["grad"])
        worst_l, worst_g = max(worst_l, e_l), max(worst_g, e_g)
        if str(key) + "/cons" in fx:
            signs.add(float(np.sign(fx[str(key) + "/cons"])))
    print(f"reference fp32 vs float64 restatement: loss {worst_l:.2e}, gradients {worst_g:.2e}")
    assert signs == {1.0, -1.0}
    assert max(worst_l, worst_g) <= MEASURED_REF_FP32, (worst_l, worst_g)
    assert max(worst_l, worst_g) >= 0.5 * MEASURED_REF_FP32, "the recorded measurement is stale"


def test_torch_composition_against_reference_fixture():
    """mswegnn.loss.loss_function on CPU tensors (the torch composition) on every case of
    fx_loss.npz: bit-equal to the reference's loss and gradient on the fixture's CPU model,
    elsewhere within FX_BOUND (4.8e-07: twice the reference's own fp32 distance from float64)."""
    from mswegnn.loss import LOSS_CALLS, loss_function
    fx = _fx()
    same = _same_cpu(fx)
    calls = LOSS_CALLS[0]
    for key in fx["cases"]:
        case = lc.fixture_case(fx, str(key))
        preds = torch.from_numpy(case["pred"]).clone().requires_grad_(True)
        data, BC = lc.fixture_data(fx, case["layout"], case["x_h"], preds=preds if case["alias"] else None)
        loss = loss_function(preds, torch.from_numpy(case["real"]), data, BC, type_loss=case["type_loss"],
                             only_where_water=case["mask"], conservation=case["cons"].get("c", 0),
                             velocity_scaler=int(case["vs"]))
        loss.backward()
        if same:
            assert lc.same_bits(loss.detach().numpy(), case["loss"]), key
            assert lc.same_bits(preds.grad.numpy(), case["grad"]), key
        else:
            assert abs(float(loss) - float(case["loss"])) <= FX_BOUND * abs(float(case["loss"])), key
            assert rel_err(preds.grad, case["grad"]) <= FX_BOUND, key
    assert LOSS_CALLS[0] == calls  # CPU tensors never count as HIP calls


def test_mutants_are_caught_by_named_cases():
    """Each wrong variant changes the record or the gradients on every case listed for it."""
    assert set(lc.KILLED_BY) == set(lc.MUTANTS) and len(lc.MUTANTS) == 12
    built = {}
    for mutant, names in lc.KILLED_BY.items():
        for name in names:
            if name not in built:
                built[name] = lc.build_case(lc.CASES[name], lc.host_launch)
            case = built[name]
            caught = False
            for tl, mask, vs in lc.OPTIONS:
                args = (case["pred"], case["real"], case["ranges"], tl, mask, vs)
                good = lc.restate(*args, **case["cons"])
                bad = lc.restate(*args, **case["cons"], mutant=mutant)
                c = case["cons"].get("c", 0.0)
                gargs = dict(g=0.25, type_loss=tl, mask=mask, c=c, area=case["cons"].get("area"),
                             node_bc=case["cons"].get("node_bc"))
                g_good = lc.gradient(case["pred"], case["real"], case["ranges"], good, **gargs)
                g_bad = lc.gradient(case["pred"], case["real"], case["ranges"], bad, mutant=mutant, **gargs)
                if not (lc.same_bits(good, bad) and lc.same_bits(g_good[0], g_bad[0])
                        and lc.same_bits(g_good[1], g_bad[1])):
                    caught = True
                    break
            assert caught, (mutant, name)


# ---------------------------------------------------------------- C ABI, host only
def _lib():
    from mswegnn import _lib as L
    return L, L.lib()


def test_abi_struct_size_and_symbols():
    """Fails on the parent: the symbols do not exist."""
    L, lib = _lib()
    assert lib.msw_struct_size(b"msw_train_loss_desc") == C.sizeof(L.MswTrainLossDesc)
    for name in ("msw_train_loss_workspace", "msw_train_loss_forward", "msw_train_loss_backward",
                 "msw_train_loss_launch"):
        assert hasattr(lib, name)
    assert lib.msw_abi_version() == 1


def test_abi_launch_arithmetic():
    from mswegnn.loss import launch
    L, lib = _lib()
    assert launch(0) == (0, 256, 0)
    for rows in (1, 255, 256, 257, 1499, 131072, 131073, 262144 + 5, 1_300_000, 2 ** 31 - 2 ** 18):
        grid, per, iters = launch(rows)
        assert (grid, per, iters) == lc.host_launch(rows)
        assert grid * per * iters >= rows and grid <= 512 and grid * per * (iters - 1) < rows
    g = C.c_int32()
    assert lib.msw_train_loss_launch(-1, C.byref(g), C.byref(g), C.byref(g)) == -1
    assert lib.msw_train_loss_launch(5, None, C.byref(g), C.byref(g)) == -1


def test_abi_invalid_arguments_are_refused_without_a_gpu():
    """Every MSW_ERR_INVALID condition of the header returns before any HIP call: the pointers are
    small integers no device call could take."""
    from mswegnn.loss import make_desc
    L, lib = _lib()
    P = 64  # a non-NULL "pointer"
    ok = dict(num_rows=100, ranges=[(0, 40), (50, 90)], type_loss="RMSE", only_where_water=True, velocity_scaler=7)
    cons = dict(conservation=0.5, num_graphs=2, seconds_per_step=7200.0, area=P, input_h=P, node_bc=P, bc=P,
                edge_bc_length=P, n_bc=2)
    n = C.c_int64(-7)
    assert lib.msw_train_loss_workspace(C.byref(make_desc(**ok)), C.byref(n)) == 0 and n.value == 4
    assert lib.msw_train_loss_workspace(C.byref(make_desc(**ok, **cons)), C.byref(n)) == 0
    ok1500 = dict(ok, num_rows=1500, ranges=[(0, 1499)])
    assert lib.msw_train_loss_workspace(C.byref(make_desc(**ok1500)), C.byref(n)) == 0 and n.value == 4 * 6

    def refused(desc, fwd=(P, P, P, P, P), bwd=(P, P, P, P, P)):
        rf = lib.msw_train_loss_forward(C.byref(desc) if desc is not None else None, *fwd, None)
        rb = lib.msw_train_loss_backward(C.byref(desc) if desc is not None else None, *bwd, None, None)
        rw = lib.msw_train_loss_workspace(C.byref(desc) if desc is not None else None, C.byref(n))
        return rf == -1 and rb == -1, rw == -1

    assert refused(None) == (True, True)
    for i in range(5):   # a NULL required pointer with a valid desc
        args = [P] * 5
        args[i] = None
        assert lib.msw_train_loss_forward(C.byref(make_desc(**ok)), *args, None) == -1
        assert lib.msw_train_loss_backward(C.byref(make_desc(**ok)), *args, None, None) == -1
    assert b"null" in lib.msw_last_error()
    assert lib.msw_train_loss_workspace(C.byref(make_desc(**ok)), None) == -1
    bad = [dict(ok, ranges=[]), dict(ok, ranges=[(0, 1)] * 65, num_rows=100),
           dict(ok, ranges=[(40, 30)]), dict(ok, ranges=[(-1, 30)]), dict(ok, ranges=[(0, 101)]),
           dict(ok, ranges=[(50, 90), (0, 40)]), dict(ok, ranges=[(0, 40), (39, 90)]),
           dict(ok, type_loss="MSE"), dict(ok, type_loss=2), dict(ok, num_rows=-1)]
    for kw in bad:
        assert refused(make_desc(**kw)) == (True, True), kw
    for kw in (dict(cons, num_graphs=0), dict(cons, area=None), dict(cons, input_h=None), dict(cons, bc=None),
               dict(cons, edge_bc_length=None), dict(cons, node_bc=None), dict(cons, n_bc=-1)):
        assert refused(make_desc(**ok, **kw)) == (True, True), kw
    d = make_desc(**ok, **dict(cons, num_graphs=0, conservation=0.0))
    assert refused(d) == (True, True)   # num_graphs < 1 whatever the coefficient
    # without the mass term its pointers are not looked at; n_bc = 0 needs no lists
    assert lib.msw_train_loss_workspace(C.byref(make_desc(**ok, area=None, n_bc=5)), C.byref(n)) == 0
    assert lib.msw_train_loss_workspace(
        C.byref(make_desc(**ok, **dict(cons, n_bc=0, bc=None, node_bc=None, edge_bc_length=None))), C.byref(n)) == 0
    d = make_desc(**ok)
    d.num_ranges = 65
    assert refused(d) == (True, True)


def test_wrapper_falls_back_to_the_composition():
    """CPU tensors, float64, and more than 64 simulations run the torch composition; the options
    keep the reference's meaning there (Data without node_ptr, Data with it, a Batch)."""
    from mswegnn.batch import Batch
    from mswegnn.loss import fine_ranges, loss_function, torch_loss_function
    case = lc.build_case(lc.CASES["five_sims"], lc.host_launch)
    p, r = torch.from_numpy(case["pred"]), torch.from_numpy(case["real"])
    b = Batch()
    b.node_ptr = torch.tensor([[s, e, e + 1] for s, e in case["ranges"]])
    b.num_graphs, b.ptr = len(case["ranges"]), torch.zeros(6, dtype=torch.long)
    assert fine_ranges(b, p.shape[0]) == [tuple(x) for x in case["ranges"]]
    for tl, mask, vs in lc.OPTIONS:
        rec = lc.restate(case["pred"], case["real"], case["ranges"], tl, mask, vs)
        for dt in (torch.float32, torch.float64):
            got = loss_function(p.to(dt), r.to(dt), b, None, tl, mask, 0, vs)
            tol = 1e-6 if dt == torch.float32 else 1e-13
            assert abs(float(got) - rec[lc.LOSS]) <= tol * abs(rec[lc.LOSS])
    one = Graph(node_ptr=torch.tensor([5, 260, 300]))
    assert fine_ranges(one, 400) == [(5, 260)] and fine_ranges(Graph(), 400) == [(0, 400)]
    got = torch_loss_function(p[:400].double(), r[:400].double(), Graph(), None, "MAE", True, 0, 7)
    rec = lc.restate(case["pred"][:400], case["real"][:400], [(0, 400)], "MAE", True, 7.0)
    assert abs(float(got) - rec[lc.LOSS]) <= 1e-13 * abs(rec[lc.LOSS])


# ---------------------------------------------------------------- the opt-in hook
HOOK_DRIVER = r'''
import json, os, sys
REF, STUBS, ROOT, PKG, ORDER = sys.argv[1:6]
sys.path[:0] = [STUBS, REF]
sys.path.append(PKG)
sys.path.append(os.path.join(ROOT, "tests"))
import numpy as np, torch
if ORDER == "train_first":
    # training.train imports models while half-initialised: the patch waits for the first model
    import training.train
    import models.gnn
    models.gnn.GNN(num_node_features=8, num_edge_features=1, hid_features=8, K=1, n_GNN_layers=1, mlp_layers=1,
                   previous_t=3, learned_residuals=True, seed=1)
else:
    import models.gnn
    import training.train
import training.loss
res = {"reference_name": training.train.loss_function is training.loss.loss_function}
if os.environ.get("MSWEGNN_FUSED_LOSS") == "1":
    import mswegnn.loss
    res["patched"] = training.train.loss_function is mswegnn.loss.loss_function
    res["kept_reference"] = training.train._reference_loss_function is training.loss.loss_function
    import loss_cases as lc
    fx = dict(np.load(os.path.join(ROOT, "tests", "golden", "fx_loss.npz")))
    same = True
    for key in ("data/RMSE_m1_v7_c0.5", "batch/MAE_m1_v7_c0.5", "batch/RMSE_m1_v7_c0.0", "single/MAE_m0_v1_c0.5"):
        case = lc.fixture_case(fx, key)
        out = []
        for fn in (training.train.loss_function, training.train._reference_loss_function):
            preds = torch.from_numpy(case["pred"]).clone().requires_grad_(True)
            data, BC = lc.fixture_data(fx, case["layout"], case["x_h"])
            if case["layout"] == "batch":   # the reference tells a Batch by its class
                from torch_geometric.data import Batch
                d = Batch(); d.__dict__.update(data.__dict__); d._data_list = [None] * data.num_graphs
                d.__dict__.pop("num_graphs"); data = d
            loss = fn(preds, torch.from_numpy(case["real"]), data, BC, type_loss=case["type_loss"],
                      only_where_water=case["mask"], conservation=case["cons"].get("c", 0), velocity_scaler=case["vs"])
            loss.backward()
            out.append((loss.detach().numpy(), preds.grad.numpy()))
        same = same and lc.same_bits(out[0][0], out[1][0]) and lc.same_bits(out[0][1], out[1][1])
    res["cpu_bit_equal"] = same
print("RESULT " + json.dumps(res))
'''


@pytest.mark.parametrize("order,fused", [("models_first", False), ("models_first", True), ("train_first", True)])
def test_fused_loss_hook_in_a_fresh_process(order, fused):
    """MSWEGNN_FUSED_LOSS=1: training.train.loss_function is mswegnn.loss.loss_function, the
    original is kept, and on the CPU both give the same bits -- whether models or training.train is
    imported first; unset, the name is untouched."""
    from test_dropin_reference import REF, STUBS
    if not os.path.isdir(os.path.join(REF, "models")):
        pytest.skip("reference checkout not present")
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", OMP_NUM_THREADS="4")
    env.pop("PYTHONPATH", None)
    env.pop("MSWEGNN_FUSED_LOSS", None)
    if fused:
        env["MSWEGNN_FUSED_LOSS"] = "1"
    p = subprocess.run([sys.executable, "-c", HOOK_DRIVER, REF, STUBS, ROOT, PKG, order], cwd=REF, env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    if fused:
        assert r["patched"] and r["kept_reference"] and r["cpu_bit_equal"], r
    else:
        assert r["reference_name"], r
