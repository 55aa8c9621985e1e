"""The HIP engine across input layouts and processor flags (tests/layout_cases.py).

The kernels carry run-time code for the layout (nnf, dyn = 2p, nstat_raw, the water-level slot
4 g + r == nstat, the window shift, the residual sum over tau < p, the BC column map) in four
written copies: decode_tail / decode_state_tail (k_base.h), k_encode, k_encode_coop, the init
kernel.  Every other GPU test runs them at p = 3, two static columns, one raw edge feature, an
edge encoder, the water level, one BC row.  Here: p = 1, 2, 3, 4, 5, 6, 8, one to sixteen static
inputs with the water level in each lane group or absent, 1 to 16 raw edge features with and
without the edge encoder, two BC rows, both type_BC, normalize / with_gradient off, at
F = 32 and (a subset) 16, 64, 50, on the MSGNN and the GNN: 31 cases.

Yardstick: the oracle with sensitised weights; tests/test_layout.py (CPU) proves that each of a
list of defects (a flag flipped, every SWEGNN output x 1.1, the window not shifted, the BC in the
other column, the water level omitted or built from the oldest h, any one input column dropped)
moves an observable asserted here by >= 1e-2, 100 x REL_TOL, and that the fp32 oracle resolves
these rollouts to REL_TOL / 10.  No defect is ever applied to the engine.
"""
import ctypes as C
import os
import warnings

import pytest
import torch

from conftest import REL_TOL, assert_rollout_parity, golden, per_step_rel, rel_err
import layout_cases as lc
import msgnn_torch as orc
from mswegnn import _lib as L
from mswegnn.batch import collate
from mswegnn.engine import EnginePlan, describe_graph, describe_model, plan_for
from mswegnn.rollout import adapt_batch_training, apply_boundary_condition, rollout_test, use_prediction

pytestmark = pytest.mark.gpu

COMBOS = lc.combos()
_cases, _default = {}, {}
WORST = {}  # combo id -> worst per-step rel error against the oracle


def _clean_env(monkeypatch):
    for k in [k for k in os.environ if k.startswith("MSW_")]:
        monkeypatch.delenv(k)


def case_of(combo):
    """-> (model, P, cfg, graph, T, the oracle's observables), built once per combo."""
    if combo not in _cases:
        case, kind, F = combo
        m, P, cfg = lc.build_model(case, kind, F)
        g, T = lc.make_graph(case, kind), lc.steps(case)
        _cases[combo] = (m, P, cfg, g, T, lc.observe(P, cfg, g, T))
    return _cases[combo]


def _run(combo, cuda, buffers=False):
    """-> dict(y, rollout, fwd / roll schedules, stats[, debug buffers]) of a fresh plan under
    the MSW_* variables set now."""
    m, P, cfg, g, T, _ = case_of(combo)
    gd = g.to(cuda)
    plan = EnginePlan(m.to(cuda), gd, cuda)
    try:
        out = {"y": plan.forward(gd.x).cpu()}
        if buffers:
            names = ("x_s", "x_d") if combo[1] == "gnn" else ("x_s", "x_d", "x_down", "x_up")
            out["buf"] = {k: plan.debug_buffer(k, combo[2]).cpu() for k in names}
        out["rollout"] = plan.rollout(gd.x, gd.BC, gd.node_BC, gd.type_BC, T).cpu()
        out["fwd"], out["roll"], out["stats"] = plan.schedule(False), plan.schedule(True), plan.stats()
        return out
    finally:
        plan.close()


def default_run(combo, cuda, monkeypatch):
    _clean_env(monkeypatch)
    if combo not in _default:
        _default[combo] = _run(combo, cuda, buffers=True)
    return _default[combo]


# ------------------------------------------------------------------ 1. one forward
@pytest.mark.parametrize("combo", COMBOS, ids=lc.combo_id)
def test_forward_and_intermediates_vs_oracle(cuda, combo, monkeypatch):
    """x_s, x_d (finest rows), x_down, x_up (msw_debug_buffer) and y of one forward."""
    m, P, cfg, g, T, ref = case_of(combo)
    run = default_run(combo, cuda, monkeypatch)
    got = lc.select(cfg, dict(run["buf"], y=run["y"]), g)
    errs = {k: rel_err(v, ref[k]) for k, v in got.items()}
    print(f"{lc.combo_id(combo)}: forward rel errors " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    assert set(errs) == set(ref) - {"rollout"}
    for k, v in got.items():
        assert v.shape == ref[k].shape, k
    assert all(e <= REL_TOL for e in errs.values()), errs
    WORST[lc.combo_id(combo)] = max(WORST.get(lc.combo_id(combo), 0.0), errs["y"])


# ------------------------------------------------------------------ 2. rollout of p + 3 steps
@pytest.mark.parametrize("combo", COMBOS, ids=lc.combo_id)
def test_rollout_vs_oracle_and_fixture(cuda, combo, monkeypatch):
    m, P, cfg, g, T, ref = case_of(combo)
    r = default_run(combo, cuda, monkeypatch)["rollout"]
    assert T == lc.layout(combo[0])["p"] + 3 and r.shape == ref["rollout"].shape
    assert ref["rollout"].abs().max() > 0.1
    e, e_ref = assert_rollout_parity(r, ref["rollout"], P, cfg, g, T, label=lc.combo_id(combo))
    print(f"{lc.combo_id(combo)}: rollout per-step rel {e:.2e}" + (f" (fp32 reference vs fp64 {e_ref:.2e})" if e_ref else ""))
    WORST[lc.combo_id(combo)] = max(WORST.get(lc.combo_id(combo), 0.0), e)
    if combo in lc.FIXTURES:  # what the reference's own rollout_test wrote
        fx = torch.from_numpy(golden(lc.fixture_name(combo))["rollout"])
        ef = per_step_rel(r, fx)
        print(f"{lc.combo_id(combo)}: rollout per-step rel {ef:.2e} against the reference's fixture")
        assert fx.abs().max() > 0.1 and ef <= REL_TOL, ef


# ------------------------------------------------------------------ 3. other schedules
def _encode(sched):
    enc = [s for s in sched if s["kind"] == "encode"]
    assert enc and sched[0]["kind"] == "encode"
    return enc[0]


def _check_identical(run, base, what):
    assert torch.equal(run["y"], base["y"]), (what, (run["y"] - base["y"]).abs().max().item())
    assert torch.equal(run["rollout"], base["rollout"]), (what, (run["rollout"] - base["rollout"]).abs().max().item())


@pytest.mark.parametrize("combo", COMBOS, ids=lc.combo_id)
def test_other_schedules_are_bit_identical(cuda, combo, monkeypatch):
    """The decoder in the last hops (decode_tail) and in the next step's encoder
    (decode_state_tail), the cooperative and the one-wave encoder, and the grid-stride encoder
    walking several chunks per workgroup: the same forward and rollout bit for bit, with the
    intended variants read back from the schedule."""
    base = default_run(combo, cuda, monkeypatch)
    nt = base["stats"]["padded_features"] // 16
    assert all(s["nt"] == nt for s in base["roll"])
    # decoder placement
    for v in ("0", "1"):
        _clean_env(monkeypatch)
        monkeypatch.setenv("MSW_DEFER_DECODE", v)
        run = _run(combo, cuda)
        assert ("dec" in _encode(run["roll"])["variant"].split()) == (v == "1"), run["roll"][0]
        assert any(s["kind"] == "decode" for s in run["fwd"]) == (v == "1")
        _check_identical(run, base, f"MSW_DEFER_DECODE={v}")
    # the other encoder (cooperative: P = NT waves per row tile, NT >= 2 only)
    was = "coop" in _encode(base["roll"])["variant"].split()
    _clean_env(monkeypatch)
    monkeypatch.setenv("MSW_ENC_COOP", "0" if was else "1")
    run = _run(combo, cuda)
    now = "coop" in _encode(run["roll"])["variant"].split()
    assert now == ((not was) and nt >= 2), (was, now, nt)
    assert ("coop" in _encode(run["fwd"])["variant"].split()) == now
    _check_identical(run, base, "MSW_ENC_COOP flipped")
    # grid-stride encoder: two workgroups walk the 64-row chunks, with and without its decoder
    for defer in ("1", "0"):
        _clean_env(monkeypatch)
        for k, v in {"MSW_GRID_CAP": "2", "MSW_ENC_COOP": "0", "MSW_DEFER_DECODE": defer}.items():
            monkeypatch.setenv(k, v)
        run = _run(combo, cuda)
        enc = _encode(run["roll"])
        words = enc["variant"].split()
        assert enc["iters"] >= 2 and enc["grid"] <= 2 and "loop" in words and "coop" not in words, enc
        assert ("dec" in words) == (defer == "1"), enc
        _check_identical(run, base, f"MSW_GRID_CAP=2 MSW_DEFER_DECODE={defer}")


# ------------------------------------------------------------------ 4. the reference's step loop
@pytest.mark.parametrize("combo", COMBOS, ids=lc.combo_id)
def test_step_loop_matches_fused_rollout(cuda, combo, monkeypatch):
    """The reference's own loop (apply_boundary_condition, forward through msw_forward,
    use_prediction) == msw_rollout with and without graph capture, bit for bit."""
    _clean_env(monkeypatch)
    m, P, cfg, g, T, ref = case_of(combo)
    p = lc.layout(combo[0])["p"]
    m = m.to(cuda)
    m.engine = "hip"
    gd = g.to(cuda)
    plan = plan_for(m, gd)
    plan.set_graph_capture(True)
    r1 = m.rollout(gd, T).clone()
    assert plan.stats()["graph_captured"] == 1
    plan.set_graph_capture(False)
    r2 = m.rollout(gd, T).clone()
    temp = gd.clone()
    preds = []
    with torch.no_grad():
        for t in range(T):
            temp.x[:, -2 * p:] = apply_boundary_condition(temp.x[:, -2 * p:], temp.BC[:, :, t], temp.node_BC,
                                                          temp.type_BC)
            y = m(temp)
            temp.x = use_prediction(temp.x, y, p)
            preds.append(y)
    r3 = torch.stack(preds, -1)
    assert plan_for(m, gd) is plan  # (the plan stays with the model's cache)
    plan.set_graph_capture(True)
    m.engine = "auto"
    assert torch.equal(r1, r2), (r1 - r2).abs().max().item()
    assert torch.equal(r1, r3), (r1 - r3).abs().max().item()
    assert torch.equal(r1.cpu(), default_run(combo, cuda, monkeypatch)["rollout"])


# ------------------------------------------------------------------ 5. extra shapes
def test_batch_of_two_meshes(cuda, monkeypatch):
    """Two meshes of different size with two BC rows each, p = 5, no water level, three raw
    edge features: the batched rollout against the oracle on the collated graph."""
    _clean_env(monkeypatch)
    case = "p5_s3_nowl_e3"
    m, P, cfg = lc.build_model(case, "msgnn", 32)
    gs = [lc.make_graph(case, seed=1), lc.make_graph(case, seed=2, n_coarse=3)]
    T = lc.steps(case)
    b = collate(gs)
    ref_graph = adapt_batch_training(b)
    assert ref_graph.node_BC.numel() == 4
    ref = orc.rollout(P, cfg, ref_graph, T)
    m = m.to(cuda)
    m.engine = "hip"
    r = rollout_test(m, b.to(cuda)).cpu()
    assert r.shape == ref.shape == (sum(g.num_nodes for g in gs), 2, T) and ref.abs().max() > 0.1
    e, _ = assert_rollout_parity(r, ref, P, cfg, ref_graph, T, label="layout batch of two")
    WORST["batch of two " + case] = e


def test_two_part_decomposition(cuda, monkeypatch):
    """A 2-part PartitionedRollout at p = 8, 15 static columns + the water level, 16 raw edge
    features: bit for bit the undivided rollout."""
    from mswegnn.partition import PartitionedRollout
    _clean_env(monkeypatch)
    combo = ("p8_s15_e16", "msgnn", 32)
    m, P, cfg, g, T, ref = case_of(combo)
    whole = default_run(combo, cuda, monkeypatch)["rollout"]
    gd = g.to(cuda)
    pr = PartitionedRollout(m.to(cuda), gd, 2, cuda)
    try:
        parts = pr.rollout(gd.x, gd.BC, gd.node_BC, gd.type_BC, T).cpu()
        again = pr.rollout(gd.x, gd.BC, gd.node_BC, gd.type_BC, T).cpu()
    finally:
        pr.close()
    assert torch.equal(parts, whole), (parts - whole).abs().max().item()
    assert torch.equal(again, whole)


def test_bc_broadcast_over_the_window(cuda, monkeypatch):
    """BC given as [n_BC, 1, T + 1] at p = 5: x_d[node_BC, c::2] = BC broadcasts the one column
    over the five slots (utils/dataset.py:496)."""
    _clean_env(monkeypatch)
    combo = ("p5_s3_nowl_e3", "msgnn", 32)
    m, P, cfg, g, T, _ = case_of(combo)
    g1 = g.clone()
    g1.BC = g.BC[:, -1:, :].clone()
    assert g1.BC.shape == (2, 1, T + 1)
    ref = orc.rollout(P, cfg, g1, T)
    full = orc.rollout(P, cfg, g, T)
    assert per_step_rel(ref, full) > 1e-2, "the broadcast series must differ from the window's"
    gd = g1.to(cuda)
    plan = EnginePlan(m.to(cuda), gd, cuda)
    try:
        r = plan.rollout(gd.x, gd.BC, gd.node_BC, gd.type_BC, T).cpu()
    finally:
        plan.close()
    assert ref.abs().max() > 0.1
    e, _ = assert_rollout_parity(r, ref, P, cfg, g1, T, label="BC broadcast p5")
    WORST["BC broadcast p5"] = e


# ------------------------------------------------------------------ 6. admission edges
def _plan_of(case, kind, F, cuda):
    m = lc.build_model(case, kind, F)[0]
    return EnginePlan(m.to(cuda), lc.make_graph(case, kind).to(cuda), cuda)


@pytest.mark.parametrize("case,F", [(dict(p=8), 32), (dict(nstat=15), 32), (dict(nstat=16, wl=False), 16),
                                    (dict(ef=16), 64), (dict(ef=16, enc=False), 16)])
def test_caps_are_accepted(cuda, case, F, monkeypatch):
    """p = 8, 16 static inputs (with and without the water level among them), 16 raw edge
    features (with the encoder; without it up to F)."""
    _clean_env(monkeypatch)
    plan = _plan_of(case, "msgnn", F, cuda)
    try:
        assert plan.stats()["hid_features"] == F and len(plan.schedule()) > 0
    finally:
        plan.close()


REFUSED = [(dict(p=9), 32, "node feature layout"),
           (dict(nstat=16), 32, "node feature layout"),            # 16 columns + the water level
           (dict(nstat=17, wl=False), 32, "node feature layout"),
           (dict(ef=17), 32, "more than 16 raw edge features"),
           (dict(ef=17, enc=False), 16, "more raw edge features than F")]


@pytest.mark.parametrize("case,F,why", REFUSED)
def test_past_the_caps_is_refused(cuda, case, F, why, monkeypatch):
    """Plans only: nothing is ever launched on a refused layout."""
    _clean_env(monkeypatch)
    for kind in ("msgnn", "gnn"):
        with pytest.raises(L.EngineError) as ei:
            _plan_of(case, kind, F, cuda)
        assert ei.value.code == L.MSW_ERR_UNSUPPORTED and why in str(ei.value), (kind, str(ei.value))


@pytest.mark.parametrize("p", [0, -1])
def test_previous_t_below_one_is_refused(cuda, p, monkeypatch):
    """previous_t < 1 (the kernels write the newest pair at columns dyn - 2, dyn - 1): refused
    when the plan is created, with MSW_ERR_UNSUPPORTED, before anything else is looked at."""
    _clean_env(monkeypatch)
    for kind in ("msgnn", "gnn"):
        m = lc.build_model("p1", kind, 32)[0]
        g = lc.make_graph("p1", kind)
        md, k1 = describe_model(m)
        gd, k2 = describe_graph(m, g)
        md.previous_t = p
        h = C.c_void_p()
        rc = L.lib().msw_plan_create(C.byref(gd), C.byref(md), cuda.index or 0, C.byref(h))
        msg = L.lib().msw_last_error().decode()
        assert rc == L.MSW_ERR_UNSUPPORTED and "previous_t" in msg and not h.value, (rc, msg)
        del k1, k2


@pytest.mark.parametrize("case,F,why", REFUSED)
def test_auto_falls_back_on_a_refused_layout(cuda, case, F, why, monkeypatch):
    """engine='auto' on each refused layout: the torch path runs (against the oracle), one
    warning, the engine's reason kept in engine_fallback_reason."""
    _clean_env(monkeypatch)
    m, P, cfg = lc.build_model(case, "msgnn", F)
    g = lc.make_graph(case)
    m = m.to(cuda)
    assert m.engine == "auto" and m.engine_fallback_reason is None
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with torch.no_grad():
            y = m(g.to(cuda)).cpu()
            r = m.rollout(g.to(cuda), 2).cpu()
    hits = [x for x in w if "HIP engine refused" in str(x.message)]
    assert len(hits) == 1 and why in str(hits[0].message), [str(x.message) for x in w]
    assert m.engine_fallback_reason and why in m.engine_fallback_reason
    assert rel_err(y, orc.forward(P, cfg, g)) <= REL_TOL
    assert per_step_rel(r, orc.rollout(P, cfg, g, 2)) <= REL_TOL


def test_report_worst_error():
    """Prints the worst error against the oracle over the layout cases run above."""
    if not WORST:
        pytest.skip("needs the parity cases of this module to have run first")
    k = max(WORST, key=WORST.get)
    print(f"layouts: worst rel error vs the oracle {WORST[k]:.2e} ({k}) over {len(WORST)} cases")
