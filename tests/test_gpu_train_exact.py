"""The training kernels (csrc/train.hip) pinned bit for bit at their tile, split-K and
grid-stride edges: mlp_apply, swegnn_apply and pool_apply -- the entries the models use -- on the
planted cases of tests/train_cases.py, every returned tensor (output, input gradients, every
parameter gradient) equal under torch.equal to the float64 restatement after its single cast to
float32.  On planted data every fp32 sum the kernels form is exact in any order and the fp64
accumulated gradients round once (train_cases.py states and asserts the bound), so any difference
is a wrong value, not rounding: a dropped row, slice, column or element shows wherever it falls,
however small its magnitude.

The same shapes then run at full precision (random normal data, normalize=True, the
transcendental activations) at the bar of tests/test_gpu_train_fuzz.py: 1e-4 per tensor against
torch's fp32 autograd, or no further from a float64 autograd than torch's fp32 result is (x2,
+1e-5).
"""
import copy

import numpy as np
import pytest
import torch

import train_cases as tc
from conftest import rel_err
from test_gpu_train_fuzz import TOL

pytestmark = pytest.mark.gpu


def assert_exact(ours, ref, what):
    """ours: name -> GPU tensor, ref: name -> float32 array; equal to the bit, else the first
    differing element with its row and column."""
    assert set(ours) == set(ref), (what, sorted(ours), sorted(ref))
    for k in sorted(ref):
        assert ours[k] is not None, (what, k, "no gradient returned")
        a, b = ours[k].detach().cpu(), torch.from_numpy(ref[k])
        assert a.dtype == torch.float32 and tuple(a.shape) == tuple(b.shape), (what, k, a.dtype, a.shape, b.shape)
        if torch.equal(a, b):
            continue
        cols = a.shape[-1] if a.dim() > 1 else 1
        a2, b2 = a.reshape(-1, cols), b.reshape(-1, cols)
        ne = (a2 != b2) | (a2.isnan() != b2.isnan())
        i = int(torch.nonzero(ne.reshape(-1))[0])
        r, c = divmod(i, a2.shape[1])
        raise AssertionError(f"{what}: {k} {tuple(a.shape)} differs at {int(ne.sum())} of {ne.numel()} elements, first "
                             f"at flat index {i} = row {r}, column {c}: kernel {a2[r, c].item()!r}, "
                             f"exact {b2[r, c].item()!r}")


def _dev(a, dev, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).to(dev)
    return t.requires_grad_(True) if grad else t


# ------------------------------------------------------------------------------------------ MLP
def hip_mlp(case, dev, seq=None):
    from mswegnn import autograd as ag
    seq = tc.build_seq(case["layers"], torch.float32).to(dev) if seq is None else seq
    x = _dev(case["x"], dev, case["need_dx"])
    assert ag.mlp_supported(seq, x)
    calls = ag.MLP_CALLS[0]
    out = ag.mlp_apply(seq, x)
    assert ag.MLP_CALLS[0] == calls + 1, "the HIP training kernels did not run"
    out.backward(_dev(case["grad_out"], dev))
    return _mlp_result(case, seq, x, out)


def _mlp_result(case, seq, x, out):
    res = {"out": out.detach()}
    if case["need_dx"]:
        res["d_x"] = x.grad
    lins = [m for m in seq if isinstance(m, torch.nn.Linear)]
    slopes = [m for m in seq if isinstance(m, torch.nn.PReLU)]
    keys = {f"dW{l}" for l, ly in enumerate(case["layers"]) if ly["train_W"]}
    keys |= {f"db{l}" for l, ly in enumerate(case["layers"]) if ly["b"] is not None and ly["train_b"]}
    res.update(tc.module_grads(keys, case["layers"], lins, slopes))
    return res


def _mlp_exact(cuda, name):
    assert_exact(hip_mlp(tc.mlp_case(name), cuda), tc.f32(tc.mlp_expected(name)), name)


@pytest.mark.parametrize("frozen", [False, True], ids=["fused_bias", "frozen_weight"])
@pytest.mark.parametrize("R", tc.ROWS)
def test_mlp_rows(cuda, R, frozen):
    """Split-K slice counts (a change at every multiple of 128, fewer slices used than asked, the
    clamp at 32768, a last slice shorter than 16 rows), row-tile tails, the slope partials over
    1 .. 256 blocks, rchunk past 256 -- with the bias gradient as the GEMM's ones column, and,
    with the first weight frozen, as column sums."""
    _mlp_exact(cuda, f"rows_{R}" + ("_frozen" if frozen else ""))


@pytest.mark.parametrize("R", [65, 257])
@pytest.mark.parametrize("pair", tc.PAIRS, ids=lambda p: f"{p[0]}x{p[1]}")
def test_mlp_widths(cuda, pair, R):
    """M / N / K tile tails, K not a multiple of 4, a second column tile, a width of 1 on either
    side, the ones column at a tile's last lane, column sums with idle threads and past 256."""
    _mlp_exact(cuda, f"pair_{pair[0]}_{pair[1]}_R{R}")


@pytest.mark.parametrize("act", ["none", "relu", "prelu"])
@pytest.mark.parametrize("bias", ["bias", "nobias"])
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_mlp_depth_bias_activation(cuda, depth, bias, act):
    _mlp_exact(cuda, f"depth{depth}_{bias}_{act}")


@pytest.mark.parametrize("name", ["frozen_33_50", "no_dx_17_15", "no_dx_frozen_65_2", "slope_one_block",
                                  "slope_256_blocks"])
def test_mlp_absent_outputs_and_slope_partials(cuda, name):
    """A frozen weight with a trainable bias, an input that needs no gradient, and the PReLU
    slope's partial sums over one block and over 256 blocks of several rounds."""
    _mlp_exact(cuda, name)


# -------------------------------------------------------------------------------------- pooling
def hip_pool(case, dev):
    from mswegnn import autograd as ag
    x = _dev(case["x"], dev, True)
    pe = torch.from_numpy(case["pool_edges"]).to(dev)
    assert ag.pool_supported(x, pe)
    calls = ag.POOL_CALLS[0]
    out = ag.pool_apply(x, pe)
    assert ag.POOL_CALLS[0] == calls + 1, "the HIP pooling kernels did not run"
    out.backward(_dev(case["grad_out"], dev))
    return {"out": out.detach(), "d_x": x.grad}


@pytest.mark.parametrize("name", list(tc.POOL_SPECS))
def test_pool(cuda, name):
    """0 .. 16 children per parent, childless parents, parentless rows, a row with two parents;
    and N * F just past one round of the grid, with checked values in the second round."""
    assert_exact(hip_pool(tc.pool_case(name), cuda), tc.f32(tc.pool_expected(name)), name)


# --------------------------------------------------------------------------------------- SWEGNN
def hip_swegnn(case, dev, lay=None):
    from mswegnn import autograd as ag
    N, F = case["x_d"].shape
    ea = case["edge_attr"]
    ef = 0 if ea is None else ea.shape[1]
    lay = tc.build_swegnn(case, torch.float32, F, ef).to(dev) if lay is None else lay
    xs, xd = _dev(case["x_s"], dev, True), _dev(case["x_d"], dev, True)
    e = _dev(ea, dev, True) if ef else None
    ei = torch.from_numpy(case["edge_index"]).to(dev)
    assert ag.supported(lay, xs, xd, e)
    calls = ag.SWEGNN_CALLS[0]
    out = ag.swegnn_apply(lay, xs, xd, ei, e)
    assert ag.SWEGNN_CALLS[0] == calls + 1, "the HIP training kernels did not run"
    out.backward(_dev(case["grad_out"], dev))
    res = {"out": out.detach(), "d_x_s": xs.grad, "d_x_d": xd.grad}
    if ef:
        res["d_edge_attr"] = e.grad
    lins = [m for m in lay.edge_mlp if isinstance(m, torch.nn.Linear)]
    slopes = [m for m in lay.edge_mlp if isinstance(m, torch.nn.PReLU)]
    keys = {f"dW{l}" for l in range(len(lins))}
    keys |= {f"db{l}" for l, ly in enumerate(case["layers"]) if ly["b"] is not None}
    res.update(tc.module_grads(keys, case["layers"], lins, slopes,
                               lay.filter_matrix if case["filters"] is not None else None))
    return res


@pytest.mark.parametrize("name", list(tc.SWEGNN_SPECS))
def test_swegnn(cuda, name):
    """F x ef x filter x gradient term x upwind on a graph with rows of in-degree 0, out-degree 0,
    an isolated row and dry rows (inactive and mixed edges); the E = 0 graph; N * F and E * F,
    E * w0 past one round of the elementwise grids."""
    assert_exact(hip_swegnn(tc.swegnn_case(name), cuda), tc.f32(tc.swegnn_expected(name)), name)


# ------------------------------------------------------------------- the shapes at full precision
SMOOTH = ["tanh", "elu", "swish", "sigmoid", "leakyrelu"]
MLP_THIRD = list(tc.MLP_SPECS)[::3]
SWEGNN_THIRD = [n for n in list(tc.SWEGNN_SPECS)[1::3] if tc.SWEGNN_SPECS[n]["E"] > 0] + ["nodes_past_cap"]
POOL_THIRD = ["pool_F50", "pool_past_cap"]


def assert_fuzz_bar(ours, ref, ref64, what):
    """tests/test_gpu_train_fuzz.py's bar: 1e-4 per tensor against torch's fp32 autograd, else no
    further from the float64 autograd than torch's fp32 result is (x2, + 1e-5)."""
    assert ours.keys() == ref.keys(), (what, sorted(ours), sorted(ref))
    bad = {k: rel_err(ours[k], ref[k]) for k in ref if not rel_err(ours[k], ref[k]) <= TOL}
    if bad:
        r64 = ref64()
        for k in list(bad):
            e_ours, e_ref = rel_err(ours[k], r64[k]), rel_err(ref[k], r64[k])
            if e_ours <= 2 * e_ref + 1e-5:
                del bad[k]
            else:
                bad[k] = (bad[k], e_ours, e_ref)
    assert not bad, (what, bad)


def _smooth_layers(case, i):
    """The case's random layers with the transcendental activations in turn."""
    return [dict(ly, act=SMOOTH[(i + l) % len(SMOOTH)]) for l, ly in enumerate(case["layers"])]


def _smooth_seq(layers, dtype):
    from models.models import activation_functions
    seq = tc.build_seq([dict(ly, act=None) for ly in layers], dtype)
    mods = []
    for lin, ly in zip(seq, layers):
        mods += [lin, activation_functions(ly["act"])]
    return torch.nn.Sequential(*mods)


@pytest.mark.parametrize("name", MLP_THIRD)
def test_mlp_full_precision(cuda, name):
    case = tc.mlp_case(name, False)
    layers = _smooth_layers(case, MLP_THIRD.index(name))
    case = dict(case, layers=layers)

    def torch_run(dtype):
        seq = _smooth_seq(layers, dtype).to(cuda)
        x = torch.from_numpy(case["x"]).to(dtype).to(cuda).requires_grad_(case["need_dx"])
        out = seq(x)
        out.backward(torch.from_numpy(case["grad_out"]).to(dtype).to(cuda))
        return _mlp_result(case, seq, x, out)
    ours = hip_mlp(case, cuda, _smooth_seq(layers, torch.float32).to(cuda))
    assert_fuzz_bar(ours, torch_run(torch.float32), lambda: torch_run(torch.float64), name)


@pytest.mark.parametrize("name", POOL_THIRD)
def test_pool_full_precision(cuda, name):
    from models.gnn import MSGNN
    case = tc.pool_case(name, False)

    def torch_run(dtype):
        x = torch.from_numpy(case["x"]).to(dtype).to(cuda).requires_grad_(True)
        coarse, fine = torch.from_numpy(case["pool_edges"]).to(cuda)
        out = MSGNN._pooling(None, x, fine, coarse, "mean", False)
        out.backward(torch.from_numpy(case["grad_out"]).to(dtype).to(cuda))
        return {"out": out.detach(), "d_x": x.grad}
    assert_fuzz_bar(hip_pool(case, cuda), torch_run(torch.float32), lambda: torch_run(torch.float64), name)


@pytest.mark.parametrize("name", SWEGNN_THIRD)
def test_swegnn_full_precision(cuda, name):
    from models.gnn import SWEGNN
    from mswegnn import autograd as ag
    from test_gpu_train_fuzz import _grads
    case, sp = tc.swegnn_case(name, False), tc.SWEGNN_SPECS[name]
    F, ef = sp["F"], sp["ef"]
    torch.manual_seed(tc.hash_name(name))
    layer = SWEGNN(F, F, ef, K=sp["K"], normalize=True, with_filter_matrix=sp["filt"], with_gradient=sp["grad"],
                   upwind_mode=sp["upwind"], n_layers=sp["depth"],
                   activation=SMOOTH[SWEGNN_THIRD.index(name) % len(SMOOTH)], bias=sp["bias"])
    ei = torch.from_numpy(case["edge_index"]).to(cuda)

    def run(lay, dtype, engine):
        t = lambda a: torch.from_numpy(a).to(dtype).to(cuda) if a is not None else None  # noqa: E731
        return _grads(lay, t(case["x_s"]), t(case["x_d"]), ei, t(case["edge_attr"]) if ef else None,
                      t(case["grad_out"]), engine)
    lay = copy.deepcopy(layer).to(cuda)
    calls = ag.SWEGNN_CALLS[0]
    ours = run(lay, torch.float32, "auto")
    assert ag.SWEGNN_CALLS[0] > calls, "the HIP training kernels did not run"
    ref = run(lay, torch.float32, "torch")
    assert_fuzz_bar(ours, ref, lambda: run(copy.deepcopy(layer).double().to(cuda), torch.float64, "torch"), name)
