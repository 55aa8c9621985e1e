"""The training kernels' yardstick (tests/train_cases.py) checked on the CPU: the numpy
restatement against torch float64 autograd of the drop-in's own modules -- an nn.Sequential with
the case's weights, models.gnn.SWEGNN with train_engine="torch", MSGNN._pooling -- equal to the
bit on planted data (both are then exact) and within 1e-12 relative on full-precision random data
(a float64 rounding allowance); the exactness bounds of every planted case; every wrong variant
caught by a named case.  tests/test_gpu_train_exact.py holds the HIP kernels to the same
restatement.
"""
import numpy as np
import pytest
import torch

import train_cases as tc

F64_TOL = 1e-12

# the largest cases run once, planted; the rest also at full precision
BIG = {"nodes_past_cap", "edges_past_cap", "pool_past_cap"}
MLP_RANDOM = [n for n in tc.MLP_SPECS if tc.MLP_SPECS[n]["R"] <= 2049]
SWEGNN_RANDOM = [n for i, n in enumerate(tc.SWEGNN_SPECS) if n not in BIG and i % 3 == 0]


def _compare(ours, ref, exact, what):
    assert set(ours) == set(ref), (what, sorted(ours), sorted(ref))
    for k in sorted(ref):
        a, b = np.asarray(ours[k], np.float64), ref[k].detach().numpy().astype(np.float64)
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        if exact:
            assert np.array_equal(a, b), (what, k, np.argwhere(a != b)[:1], a[a != b][:1], b[a != b][:1])
        else:
            den = max(float(np.abs(b).max(initial=0.0)), 1e-300)
            err = float(np.abs(a - b).max(initial=0.0)) / den
            assert err <= F64_TOL, (what, k, err)


def torch_mlp(case):
    seq = tc.build_seq(case["layers"], torch.float64)
    x = torch.from_numpy(case["x"]).requires_grad_(case["need_dx"])
    out = seq(x)
    if out.requires_grad:
        out.backward(torch.from_numpy(case["grad_out"]))
    res = {"out": out.detach()}
    if case["need_dx"]:
        res["d_x"] = x.grad
    lins = [m for m in seq if isinstance(m, torch.nn.Linear)]
    slopes = [m for m in seq if isinstance(m, torch.nn.PReLU)]
    keys = {f"dW{l}" for l, ly in enumerate(case["layers"]) if ly["train_W"]}
    keys |= {f"db{l}" for l, ly in enumerate(case["layers"]) if ly["b"] is not None and ly["train_b"]}
    res.update(tc.module_grads(keys, case["layers"], lins, slopes))
    return res


def torch_swegnn(case):
    N, F = case["x_d"].shape
    ea = case["edge_attr"]
    ef = 0 if ea is None else ea.shape[1]
    lay = tc.build_swegnn(case, torch.float64, F, ef)
    lay.train_engine = "torch"
    xs = torch.from_numpy(case["x_s"]).requires_grad_(True)
    xd = torch.from_numpy(case["x_d"]).requires_grad_(True)
    e = torch.from_numpy(ea).requires_grad_(True) if ef else None
    out = lay(xs, xd, torch.from_numpy(case["edge_index"]), e)
    out.backward(torch.from_numpy(case["grad_out"]))
    res = {"out": out.detach(), "d_x_s": xs.grad if xs.grad is not None else torch.zeros_like(xs), "d_x_d": xd.grad}
    if ef:
        res["d_edge_attr"] = e.grad
    lins = [m for m in lay.edge_mlp if isinstance(m, torch.nn.Linear)]
    slopes = [m for m in lay.edge_mlp if isinstance(m, torch.nn.PReLU)]
    keys = {f"dW{l}" for l in range(len(lins))}
    keys |= {f"db{l}" for l, ly in enumerate(case["layers"]) if ly["b"] is not None}
    g = tc.module_grads(keys, case["layers"], lins, slopes, lay.filter_matrix if case["filters"] is not None else None)
    res.update({k: v if v is not None else torch.zeros(_shape_of(k, case)) for k, v in g.items()})
    return res


def _shape_of(key, case):
    """A parameter no edge reaches gets no gradient from autograd (E = 0): zeros of its shape."""
    l = int("".join(ch for ch in key if ch.isdigit()))
    if key.startswith("dW"):
        return case["layers"][l]["W"].shape
    if key.startswith("db"):
        return case["layers"][l]["b"].shape
    if key.startswith("dslope"):
        return (1,)
    return case["filters"][l].shape


def torch_pool(case):
    from models.gnn import MSGNN
    x = torch.from_numpy(case["x"]).requires_grad_(True)
    coarse, fine = torch.from_numpy(case["pool_edges"])
    out = MSGNN._pooling(None, x, fine, coarse, "mean", False)
    out.backward(torch.from_numpy(case["grad_out"]))
    return {"out": out.detach(), "d_x": x.grad}


TORCH = {"mlp": (tc.mlp_case, torch_mlp), "swegnn": (tc.swegnn_case, torch_swegnn), "pool": (tc.pool_case, torch_pool)}


def _check(family, name, planted):
    case, run = TORCH[family]
    bound = tc.Bound() if planted else None
    ours = tc.EXPECTED[family](name, planted, None, bound)
    if planted:
        bound.check()
        for k, v in ours.items():   # the single cast loses nothing but the fp64-accumulated results' tail
            if k[:2] not in ("dW", "db", "ds", "df"):
                assert np.array_equal(v.astype(np.float32).astype(np.float64), v), (name, k)
    _compare(ours, run(case(name, planted)), planted, (family, name))


@pytest.mark.parametrize("name", list(tc.MLP_SPECS))
def test_mlp_restatement_equals_torch_float64_on_planted_data(name):
    _check("mlp", name, True)


@pytest.mark.parametrize("name", MLP_RANDOM)
def test_mlp_restatement_matches_torch_float64_at_full_precision(name):
    _check("mlp", name, False)


@pytest.mark.parametrize("name", list(tc.SWEGNN_SPECS))
def test_swegnn_restatement_equals_torch_float64_on_planted_data(name):
    _check("swegnn", name, True)


@pytest.mark.parametrize("name", SWEGNN_RANDOM)
def test_swegnn_restatement_matches_torch_float64_at_full_precision(name):
    _check("swegnn", name, False)


@pytest.mark.parametrize("name", list(tc.POOL_SPECS))
def test_pool_restatement_equals_torch_float64_on_planted_data(name):
    _check("pool", name, True)


@pytest.mark.parametrize("name", [n for n in tc.POOL_SPECS if n not in BIG])
def test_pool_restatement_matches_torch_float64_at_full_precision(name):
    _check("pool", name, False)


def test_cases_hold_what_they_name():
    """The features the exact comparison is meant to see are in the data."""
    assert tc.splits_for(2049) == 16 and tc.used_splits(2049) == 15 and 2049 % tc.kchunk_for(2049) == 33
    assert tc.splits_for(32767) == 255 and tc.splits_for(32768) == 256 == tc.splits_for(65537)
    assert [tc.splits_for(r) for r in (255, 256, 257, 383, 385)] == [1, 2, 2, 2, 3]
    assert tc.rchunk_for(65535) == 256 and tc.rchunk_for(65537) == 257
    c = tc.swegnn_case("F16_ef0_filt_grad")
    row, col = c["edge_index"]
    N = c["x_d"].shape[0]
    indeg, outdeg = np.bincount(col, minlength=N), np.bincount(row, minlength=N)
    assert (indeg == 0).any() and (outdeg == 0).any() and ((indeg == 0) & (outdeg == 0)).any()
    assert ((indeg == 0) & (outdeg > 0)).any() and ((outdeg == 0) & (indeg > 0)).any()
    nz = c["x_d"].sum(1) != 0
    assert (~nz[row] & ~nz[col]).any() and (nz[row] ^ nz[col]).any() and (nz[row] & nz[col]).any()
    for name in ("nodes_past_cap", "edges_past_cap"):
        sp = tc.SWEGNN_SPECS[name]
        assert max(sp["N"], sp["E"]) * sp["F"] > tc.CAP
    c = tc.swegnn_case("nodes_past_cap")
    assert (c["edge_index"] * 64 >= tc.CAP).any() and tc.SWEGNN_SPECS["nodes_past_cap"]["E"] <= 2000
    p = tc.pool_case("pool_F16")
    cnt = np.bincount(p["pool_edges"][0], minlength=300)
    assert sorted(set(cnt[40:57])) == list(range(17))
    assert (np.bincount(p["pool_edges"][1], minlength=300) == 2).any()
    p = tc.pool_case("pool_past_cap")
    assert p["x"].size > tc.CAP
    assert (p["pool_edges"][1] * 64 >= tc.CAP).any() and (p["pool_edges"][0] * 64 >= tc.CAP).all()
    e = tc.pool_expected("pool_past_cap")
    assert np.count_nonzero(e["out"].reshape(-1)[tc.CAP:]) > 1000
    assert np.count_nonzero(e["d_x"].reshape(-1)[tc.CAP:]) > 100


@pytest.mark.parametrize("variant", tc.VARIANTS)
def test_every_wrong_variant_is_caught(variant):
    """Each wrong variant of the restatement changes a compared float32 tensor on each of its
    named cases -- and leaves the cases alone whose shape gives it nothing to get wrong."""
    for family, name in tc.VARIANT_CASES[variant]:
        good = tc.f32(tc.EXPECTED[family](name))
        bad = tc.f32(tc.EXPECTED[family](name, True, variant))
        assert good.keys() == bad.keys()
        differ = [k for k in good if not np.array_equal(good[k], bad[k], equal_nan=True)]
        assert differ, (variant, family, name)


def test_variants_are_the_issue_twelve():
    assert len(tc.VARIANTS) == 12 and set(tc.VARIANT_CASES) == set(tc.VARIANTS)
    for cases in tc.VARIANT_CASES.values():
        for family, name in cases:
            assert name in tc.SPECS[family]
