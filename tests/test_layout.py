"""Input layouts and processor flags on the CPU (tests/layout_cases.py): the oracle against
fixtures the reference itself wrote at p = 1, 4, 5 and for the GNN, the drop-in's torch path
against the oracle at every case, and the sensitivity gate of tests/test_gpu_layout.py.

The gate: a comparison at REL_TOL proves something only if a defect moves what is compared by
much more than REL_TOL.  With the seeded init a 10 % error in every processor can move a rollout
by 1.7e-4, so the cases carry sensitised weights (layout_cases.sensitize), and every defect of
layout_cases.defects -- applied to the oracle's Python or to its inputs, never to the engine --
must move an observable the GPU test asserts by >= 1e-2, 100 x REL_TOL.  A case that misses the
threshold gets other weights or inputs; the threshold stays.
"""
import numpy as np
import pytest
import torch

from conftest import REL_TOL, golden, graph_digest, per_step_rel
import layout_cases as lc
import msgnn_torch as orc
import test_oracle_golden as tog

COMBOS = lc.combos()
_cache = {}


@pytest.fixture(autouse=True)
def _threads():
    torch.set_num_threads(min(8, torch.get_num_threads()))


def case_of(combo):
    """-> (model, P, cfg, graph, T, the oracle's observables), built once per combo."""
    if combo not in _cache:
        case, kind, F = combo
        m, P, cfg = lc.build_model(case, kind, F)
        g, T = lc.make_graph(case, kind), lc.steps(case)
        _cache[combo] = (m, P, cfg, g, T, lc.observe(P, cfg, g, T))
    return _cache[combo]


def test_case_table():
    """The cases the issue names, at the slots they are named for."""
    C = lc.CASES
    assert len(COMBOS) == 31 and len(set(COMBOS)) == 31
    wl_slot = {k: c["nstat"] for k, c in C.items() if c["wl"]}  # 4 g + r == nstat_raw
    assert wl_slot["p3_s3"] == 3 and wl_slot["p3_s4_raw1"] == 4 and wl_slot["p8_s15_e16"] == 15
    assert wl_slot["p2_s1"] == 1 and wl_slot["p1"] == 2 and wl_slot["p6_s9"] == 9
    assert {s // 4 for s in wl_slot.values()} == {0, 1, 2, 3}, "a lane group without a water-level case"
    assert C["p8_s15_e16"]["p"] * 2 == 16 and C["p8_s15_e16"]["ef"] == 16
    assert C["p4_s16_nowl_raw5"]["nstat"] == 16 and not C["p4_s16_nowl_raw5"]["wl"]
    assert {c["p"] for c in C.values()} == {1, 2, 3, 4, 5, 6, 8}
    assert {c["type_bc"] for c in C.values()} == {1, 2} and C["p5_s3_nowl_e3"]["nbc"] == 2
    assert not C["p3_s4_raw1"]["enc"] and not C["p4_s16_nowl_raw5"]["enc"]
    for case in C:
        g = lc.make_graph(case)
        assert g.x.shape == (171, C[case]["nstat"] + 2 * C[case]["p"])
        assert g.edge_attr.shape[1] == C[case]["ef"] and g.node_BC.numel() == C[case]["nbc"]
        nstat = C[case]["nstat"]
        assert (g.x[:, nstat:] != 0).any(0).all(), "a dynamic column is all dry"


@pytest.mark.parametrize("combo", lc.FIXTURES, ids=lc.combo_id)
def test_oracle_vs_reference_fixture(combo):
    """The oracle reproduces what the reference's own modules and rollout_test gave
    (oracle/gen_golden_layout.py): bit for bit on the generating CPU model, 1e-5 per step
    elsewhere (tests/test_oracle_golden.py's bar)."""
    fx = golden(lc.fixture_name(combo))
    m, P, cfg, g, T, ref = case_of(combo)
    assert np.array_equal(graph_digest(g), fx["digest"]), "the case's graph drifted"
    assert float(fx["amp"]) == lc.AMP
    W = {k[3:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("w__")}
    assert W.keys() == P.keys()
    for k in P:
        assert torch.equal(W[k], P[k]), k  # seeded init + sensitize: the fixture's own weights
    same_cpu = str(fx["cpu"]) == tog._cpu_model()
    for got, want in ((orc.forward(W, cfg, g), fx["y"]), (orc.rollout(W, cfg, g, T), fx["rollout"])):
        want = torch.from_numpy(want)
        if same_cpu:
            assert torch.equal(got, want), (got - want).abs().max().item()
        else:
            assert per_step_rel(got.reshape(got.shape[0], 2, -1), want.reshape(want.shape[0], 2, -1)) <= 1e-5
    assert fx["rollout"].shape[-1] == T and np.abs(fx["rollout"]).max() > 0.1


@pytest.mark.parametrize("combo", COMBOS, ids=lc.combo_id)
def test_dropin_torch_path_equals_oracle(combo):
    m, P, cfg, g, T, ref = case_of(combo)
    with torch.no_grad():
        y, r = m(g), m.rollout(g, T)
    assert torch.equal(y, ref["y"]), (y - ref["y"]).abs().max().item()
    assert torch.equal(r, ref["rollout"]), (r - ref["rollout"]).abs().max().item()
    assert ref["rollout"].abs().max() > 0.1


@pytest.mark.parametrize("combo", COMBOS, ids=lc.combo_id)
def test_reference_resolves_the_rollout(combo):
    """The fp32 oracle stays within REL_TOL / 10 per step of float64 arithmetic: the bar of the
    GPU test is not spent on the reference's own rounding (filters x 4 instead of x 3 fail this:
    the rollouts then amplify rounding tenfold per step)."""
    m, P, cfg, g, T, ref = case_of(combo)
    P64 = {k: v.double() for k, v in P.items()}
    g64 = g.clone()
    for k in ("x", "edge_attr", "BC"):
        setattr(g64, k, getattr(g, k).double())
    e = per_step_rel(ref["rollout"], orc.rollout(P64, cfg, g64, T).float())
    print(f"{lc.combo_id(combo)}: fp32 oracle vs float64, per step {e:.2e}")
    assert e <= REL_TOL / 10, e


@pytest.mark.parametrize("combo", COMBOS, ids=lc.combo_id)
def test_sensitivity_gate(combo):
    """Every defect moves an asserted observable by >= 1e-2 (forward observables first, the
    rollout where they do not suffice: the window and BC defects show there only)."""
    case = combo[0]
    m, P, cfg, g, T, ref = case_of(combo)
    weakest = {}
    for d in lc.defects(case):
        s, k = lc.distance(lc.observe(P, cfg, g, T, d, rollout=False), ref)
        if s < lc.SENSITIVITY:
            s, k = lc.distance(lc.observe(P, cfg, g, T, d), ref)
        if d[0] not in weakest or s < weakest[d[0]][0]:
            weakest[d[0]] = (s, k, d)
    print(f"{lc.combo_id(combo)}: weakest sensitivity per defect kind (filters x {lc.AMP:g}): "
          + ", ".join(f"{n} {s:.2e} on {k}" + (f" (column {d[1]})" if len(d) > 1 else "")
                      for n, (s, k, d) in weakest.items()))
    miss = {n: v for n, v in weakest.items() if v[0] < lc.SENSITIVITY}
    assert not miss, miss
    kinds = {"normalize", "with_gradient", "swegnn_x1.1", "bc_other_type", "static", "dynamic", "edge"}
    if lc.CASES[case]["p"] > 1:
        kinds.add("window_not_shifted")
    if lc.CASES[case]["wl"]:
        kinds |= {"wl_omitted"} | ({"wl_from_oldest_h"} if lc.CASES[case]["p"] > 1 else set())
    assert set(weakest) == kinds
