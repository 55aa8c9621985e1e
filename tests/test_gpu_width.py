"""Hidden widths 33..63 on the HIP engine: zero-padded to 64 on the NT = 4 kernels.

The yardstick is the oracle (oracle/msgnn_torch.py, any width) on seeded models, REL_TOL per
step through assert_rollout_parity; tests/test_width_embed.py's ``embed`` gives the 64-wide twin
a padded plan must equal bit for bit.  Meshes: mesh_config("tiny") and "small", T = 6 from a wet
state unless a test says otherwise.
"""
import copy
import os
import warnings

import pytest
import torch

from conftest import REL_TOL, assert_rollout_parity, build_gnn, build_msgnn, per_step_rel, rel_err, state_dict_of
import msgnn_torch as orc
from mswegnn import _lib as L
from mswegnn.batch import collate
from mswegnn.engine import EnginePlan, plan_for
from mswegnn.mesh import make_multiscale_mesh, make_single_scale_mesh, mesh_config, wet_state
from mswegnn.rollout import rollout_test
from test_irregular_mesh import GPU_SEEDS, irregular
from test_width_embed import embed, gnn_case, msgnn_case, tiny_mesh

pytestmark = pytest.mark.gpu

T = 6

# name -> (scales, F, (builder, oracle cfg)); every activation here has f(0) = 0
CASES = {
    "K2_F50": (4, 50, msgnn_case(4, 50, 2)),      # the published F = 50 rows (K2 .. K5): both ends
    "K5_F50": (4, 50, msgnn_case(4, 50, 5)),
    "K135_F33": (3, 33, msgnn_case(3, 33, [1, 3, 5])),
    "K3_F63": (2, 63, msgnn_case(2, 63, 3)),
    "noskip_F50": (3, 50, msgnn_case(3, 50, 2, skip_connections=False)),
    "mlp1_F50": (3, 50, msgnn_case(3, 50, 2, mlp_layers=1)),
    "mlp4_F50": (3, 50, msgnn_case(3, 50, 2, mlp_layers=4)),
    "GNN_F50": (1, 50, gnn_case(50, mlp_layers=2)),
}

_meshes, _oracle, _native = {}, {}, {}
WORST = {}  # case -> per-step rel error against the oracle (printed by the last test)


def _clean_env(monkeypatch):
    for k in [k for k in os.environ if k.startswith("MSW_")]:
        monkeypatch.delenv(k)


def _mesh(S):
    if S not in _meshes:
        _meshes[S] = tiny_mesh(S)
    return _meshes[S]


def _ref(name):
    """The oracle's forward and T-step rollout of a case, computed once."""
    if name not in _oracle:
        S, F, (build, cfg) = CASES[name]
        P, g = state_dict_of(build()), _mesh(S)
        _oracle[name] = (P, orc.forward(P, cfg(), g), orc.rollout(P, cfg(), g, T))
    return _oracle[name]


def _run(model, g, cuda, T=T):
    """-> (forward, rollout, schedule, stats) of a fresh plan under the MSW_* variables set now."""
    plan = EnginePlan(model.to(cuda), g.to(cuda), cuda)
    try:
        gd = g.to(cuda)
        y = plan.forward(gd.x).cpu()
        r = plan.rollout(gd.x, gd.BC, gd.node_BC, gd.type_BC, T).cpu()
        return y, r, plan.schedule(), plan.stats()
    finally:
        plan.close()


def _hip_native(name, cuda, monkeypatch):
    _clean_env(monkeypatch)
    if name not in _native:
        S, F, (build, cfg) = CASES[name]
        _native[name] = _run(build(), _mesh(S), cuda)
    return _native[name]


# ------------------------------------------------------------------ 1. admission
def test_admission(cuda, monkeypatch):
    """F = 50 builds a plan (refused before: the test that shows the feature): logical width 50,
    row width 64, the schedule of its embedded 64-wide twin line by line; 24, 31 and 65 stay
    refused with MSW_ERR_UNSUPPORTED."""
    _clean_env(monkeypatch)
    S, F, (build, cfg) = CASES["K2_F50"]
    g = _mesh(S).to(cuda)
    m = build()
    plan = EnginePlan(m.to(cuda), g, cuda)
    twin = EnginePlan(build(64, embed(state_dict_of(m), F, 64)).to(cuda), g, cuda)
    try:
        st = plan.stats()
        assert st["hid_features"] == 50 and st["padded_features"] == 64, st
        st64 = twin.stats()
        assert st64["hid_features"] == 64 and st64["padded_features"] == 64, st64
        for rollout in (True, False):
            a, b = plan.schedule(rollout), twin.schedule(rollout)
            assert len(a) == len(b) and len(a) > 0
            for la, lb in zip(a, b):
                assert la == lb, (la, lb)
            assert all(s["nt"] == 4 for s in a)
    finally:
        plan.close()
        twin.close()
    for bad in (24, 31, 65):
        with pytest.raises(L.EngineError) as ei:
            EnginePlan(build_msgnn(4, bad, 2).to(cuda), g, cuda)
        assert ei.value.code == L.MSW_ERR_UNSUPPORTED, (bad, ei.value)
        assert "32..64" in str(ei.value), str(ei.value)
    with pytest.raises(L.EngineError) as ei:
        EnginePlan(build_gnn(24, 2, 2, 1).to(cuda), make_single_scale_mesh(n_coarse=2, refinements=2, T=2).to(cuda), cuda)
    assert ei.value.code == L.MSW_ERR_UNSUPPORTED


# ------------------------------------------------------------------ 2. oracle parity
@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_parity(cuda, name, monkeypatch):
    S, F, (build, cfg) = CASES[name]
    P, y_ref, r_ref = _ref(name)
    y, r, sched, st = _hip_native(name, cuda, monkeypatch)
    assert st["hid_features"] == F and st["padded_features"] == 64 and all(s["nt"] == 4 for s in sched)
    assert r_ref.abs().max() > 0.1
    ey = rel_err(y, y_ref)
    e, e_ref = assert_rollout_parity(r, r_ref, P, cfg(), _mesh(S), T, label=name)
    WORST[name] = max(ey, e)
    print(f"{name}: forward rel {ey:.2e}, rollout per-step rel {e:.2e}"
          + (f" (fp32 reference vs fp64 {e_ref:.2e})" if e_ref else ""))
    assert ey <= REL_TOL, (name, ey)


def test_k4_f50_48_steps_on_small(cuda, monkeypatch):
    """The published K4_F50 shape over a 48-step rollout of `small`."""
    _clean_env(monkeypatch)
    build, cfg = msgnn_case(4, 50, 4)
    g = wet_state(make_multiscale_mesh(**mesh_config("small"), T=48), seed=2)
    m = build()
    P = state_dict_of(m)
    ref = orc.rollout(P, cfg(), g, 48)
    _, r, _, st = _run(m, g, cuda, T=48)
    assert st["rollout_steps"] == 48
    e, e_ref = assert_rollout_parity(r, ref, P, cfg(), g, 48, label="K4_F50 small T=48")
    WORST["K4_F50 small T=48"] = e
    print(f"K4_F50 small, 48 steps: per-step rel {e:.2e}" + (f" (fp32 reference vs fp64 {e_ref:.2e})" if e_ref else ""))


def test_intermediates_vs_oracle(cuda, monkeypatch):
    """x_s, x_d, x_down, x_up of one forward (msw_debug_buffer with the logical F = 50: [N][50])
    against the oracle's: the encoders' outputs and every processor's output on its scale."""
    _clean_env(monkeypatch)
    S, F, (build, cfg) = CASES["K2_F50"]
    g, m = _mesh(S), build()
    P, c = state_dict_of(m), cfg()
    outs = {}
    real = orc.swegnn

    def spy(P_, prefix, x_s, x_d, *a, **kw):
        out = real(P_, prefix, x_s, x_d, *a, **kw)
        outs[prefix] = out
        return out

    monkeypatch.setattr(orc, "swegnn", spy)
    orc.forward(P, c, g)
    monkeypatch.setattr(orc, "swegnn", real)
    mask = orc.create_scale_mask(g.x.shape[0], S, g.node_ptr)
    xs_in = torch.cat((g.x[:, :2], (g.x[:, 1] + g.x[:, -2]).unsqueeze(-1)), 1)
    xs_ref = orc.mlp(P, "static_node_encoder", xs_in, 3, "prelu")
    xd_ref = orc.mlp(P, "dynamic_node_encoder", g.x[:, 2:], 3, "prelu")
    x_down = sum(outs[f"gnn_processor.{i}"] * (mask == i)[:, None] for i in range(S - 1))
    x_up = sum(outs[f"gnn_processor.{S - 1 + i}"] * (mask == S - 1 - i)[:, None] for i in range(S))
    plan = EnginePlan(m.to(cuda), g.to(cuda), cuda)
    try:
        plan.forward(g.x.to(cuda))
        got = {k: plan.debug_buffer(k, F).cpu() for k in ("x_s", "x_d", "x_down", "x_up")}
    finally:
        plan.close()
    fine = mask == 0
    below = mask < S - 1
    assert all(v.shape == (g.x.shape[0], F) for v in got.values())
    assert rel_err(got["x_s"], xs_ref) <= REL_TOL
    assert rel_err(got["x_d"][fine], xd_ref[fine]) <= REL_TOL
    assert rel_err(got["x_down"][below], x_down[below]) <= REL_TOL
    assert rel_err(got["x_up"], x_up) <= REL_TOL


# ------------------------------------------------------------------ 3. bit identity to the twin
@pytest.mark.parametrize("name", sorted(CASES))
def test_bit_identical_to_embedded_twin(cuda, name, monkeypatch):
    """Padding is exactly zero-embedding: the F-wide model and its 64-wide twin give the same
    forward and rollout on the engine, bit for bit."""
    S, F, (build, cfg) = CASES[name]
    y, r, sched, _ = _hip_native(name, cuda, monkeypatch)
    twin = build(64, embed(state_dict_of(build()), F, 64))
    y64, r64, sched64, st64 = _run(twin, _mesh(S), cuda)
    assert st64["hid_features"] == 64 and sched == sched64
    assert torch.equal(y, y64), (y - y64).abs().max().item()
    assert torch.equal(r, r64), (r - r64).abs().max().item()


# ------------------------------------------------------------------ 4. activations
ACTS = ["prelu", "relu", "leakyrelu", "elu", "swish", "sigmoid", "tanh"]


def _not_the_unmasked_twin(build, cfg, F, g, ref, e, label):
    """Sigmoid: the embedded twin on the oracle IS the model with every pad column left at
    sigmoid(0) = 0.5 (they enter the norm of s_ij).  With seeded weights it leaves the native
    rollout by d ~ 1e-5, inside REL_TOL, so REL_TOL alone would not see a missing mask: the
    engine must also sit at least four times closer to the native model than that twin does."""
    d = per_step_rel(orc.rollout(embed(state_dict_of(build()), F, 64), cfg(64), g, T), ref)
    print(f"{label}: the unmasked (embedded) twin leaves the native oracle by {d:.2e}, the engine by {e:.2e}")
    assert d > 1e-6, (label, d)
    assert e <= d / 4, (label, e, d)


@pytest.mark.parametrize("act", ACTS)
def test_activations_at_f40(cuda, act, monkeypatch):
    """Every mlp_activation at a padded width against the oracle.  Sigmoid is the one with
    f(0) != 0: a pad column left at 0.5 would enter the norm of s_ij."""
    _clean_env(monkeypatch)
    build, cfg = msgnn_case(3, 40, 2, mlp_activation=act)
    g, m = _mesh(3), build()
    P = state_dict_of(m)
    ref = orc.rollout(P, cfg(), g, T)
    y, r, sched, st = _run(m, g, cuda)
    assert st["padded_features"] == 64 and all(s["prelu"] == (act == "prelu") for s in sched if s["kind"] != "exchange")
    ey = rel_err(y, orc.forward(P, cfg(), g))
    e, _ = assert_rollout_parity(r, ref, P, cfg(), g, T, label=f"F40 {act}")
    WORST[f"F40 {act}"] = max(ey, e)
    print(f"F40 {act}: forward rel {ey:.2e}, rollout per-step rel {e:.2e}")
    assert ey <= REL_TOL
    if act == "sigmoid":
        _not_the_unmasked_twin(build, cfg, 40, g, ref, e, "F40 sigmoid")


@pytest.mark.parametrize("mlp_layers", [1, 2])
def test_sigmoid_gnn_at_f40(cuda, mlp_layers, monkeypatch):
    """The GNN with sigmoid as mlp_activation and gnn_activation: the layer outputs a later
    layer reads as x_d are sigmoid rows (mlp_layers = 1: s_ij is the first layer's output)."""
    _clean_env(monkeypatch)
    build, cfg = gnn_case(40, K=2, n_layers=2, mlp_layers=mlp_layers, mlp_activation="sigmoid",
                          gnn_activation="sigmoid")
    g, m = _mesh(1), build()
    P = state_dict_of(m)
    ref = orc.rollout(P, cfg(), g, T)
    y, r, _, st = _run(m, g, cuda)
    assert st["padded_features"] == 64
    ey = rel_err(y, orc.forward(P, cfg(), g))
    e, _ = assert_rollout_parity(r, ref, P, cfg(), g, T, label=f"GNN F40 sigmoid mlp{mlp_layers}")
    WORST[f"GNN F40 sigmoid mlp{mlp_layers}"] = max(ey, e)
    print(f"GNN F40 sigmoid mlp_layers={mlp_layers}: forward rel {ey:.2e}, rollout per-step rel {e:.2e}")
    assert ey <= REL_TOL
    if mlp_layers == 1:  # two layers: the twin itself stays within 5e-7 here, nothing to tell apart
        _not_the_unmasked_twin(build, cfg, 40, g, ref, e, "GNN F40 sigmoid mlp1")


def test_all_dry_start_stays_dry(cuda, monkeypatch):
    """An all-dry state without inflow gives an all-zero rollout at a padded width."""
    _clean_env(monkeypatch)
    S, F, (build, cfg) = CASES["K2_F50"]
    g = make_multiscale_mesh(**mesh_config("tiny"), T=T)
    g.BC = torch.zeros_like(g.BC)
    assert g.x[:, -6:].abs().max() == 0
    _, r, _, _ = _run(build(), g, cuda)
    assert r.abs().max() == 0
    assert orc.rollout(state_dict_of(build()), cfg(), g, T).abs().max() == 0


# ------------------------------------------------------------------ 5. every path at a padded width
def test_batch_of_two(cuda, monkeypatch):
    _clean_env(monkeypatch)
    build, cfg = msgnn_case(4, 50, 2)
    gs = [wet_state(make_multiscale_mesh(**mesh_config("small"), T=T), seed=4),
          wet_state(make_multiscale_mesh(**mesh_config("tiny"), seed=5, T=T), seed=5)]
    m = build()
    P = state_dict_of(m)
    m = m.to(cuda)
    m.engine = "hip"
    r = rollout_test(m, collate(gs).to(cuda)).cpu()
    assert r.shape == (sum(g.num_nodes for g in gs), 2, T)
    a = 0
    for i, g in enumerate(gs):
        e, _ = assert_rollout_parity(r[a:a + g.num_nodes], orc.rollout(P, cfg(), g, T), P, cfg(), g, T,
                                     label=f"F50 batch member {i}")
        WORST[f"F50 batch member {i}"] = e
        a += g.num_nodes


def test_two_way_decomposition(cuda, monkeypatch):
    """msw_plan_create_part / msw_group_rollout at F = 50: bit for bit the undivided rollout,
    replayed from the group's graphs and eager."""
    from mswegnn.partition import PartitionedRollout
    _clean_env(monkeypatch)
    build, _ = msgnn_case(4, 50, 2)
    g = wet_state(make_multiscale_mesh(**mesh_config("small"), T=T), seed=4)
    m = build()
    _, whole, _, _ = _run(m, g, cuda)
    gd = g.to(cuda)
    pr = PartitionedRollout(m.to(cuda), gd, 2, cuda)
    try:
        assert all(pl.stats()["padded_features"] == 64 and pl.stats()["hid_features"] == 50 for pl in pr.plans)
        graphed = pr.rollout(gd.x, gd.BC, gd.node_BC, gd.type_BC, T).cpu()
        again = pr.rollout(gd.x, gd.BC, gd.node_BC, gd.type_BC, T).cpu()
        L.check(L.lib().msw_set_group_graph(pr.plans[0]._h, 0))
        eager = pr.rollout(gd.x, gd.BC, gd.node_BC, gd.type_BC, T).cpu()
    finally:
        pr.close()
    assert torch.equal(graphed, whole), (graphed - whole).abs().max().item()
    assert torch.equal(again, whole) and torch.equal(eager, whole)


def test_irregular_small(cuda, monkeypatch):
    _clean_env(monkeypatch)
    build, cfg = msgnn_case(4, 50, 2)
    g = irregular("small", GPU_SEEDS[0], wet=4, T=T)[0]
    m = build()
    P = state_dict_of(m)
    y, r, _, _ = _run(m, g, cuda)
    ey = rel_err(y, orc.forward(P, cfg(), g))
    e, _ = assert_rollout_parity(r, orc.rollout(P, cfg(), g, T), P, cfg(), g, T, label="F50 irregular small")
    WORST["F50 irregular small"] = max(ey, e)
    assert ey <= REL_TOL


KNOBS = ["MSW_POOL_FUSE=0", "MSW_UNPOOL_FUSE=0", "MSW_COOP_WAVES=0", "MSW_HOP_ROWS=2", "MSW_DEFER_DECODE=0",
         "MSW_DEFER_DECODE=1"]


@pytest.mark.parametrize("knob", KNOBS)
def test_schedule_switches_are_bit_identical(cuda, knob, monkeypatch):
    y, r, sched, _ = _hip_native("K5_F50", cuda, monkeypatch)
    k, v = knob.split("=")
    monkeypatch.setenv(k, v)
    S, F, (build, _) = CASES["K5_F50"]
    y2, r2, sched2, _ = _run(build(), _mesh(S), cuda)
    if knob not in ("MSW_UNPOOL_FUSE=0", "MSW_DEFER_DECODE=1"):  # the defaults at NT = 4 on this mesh
        assert sched2 != sched, knob
    assert torch.equal(y2, y), (knob, (y2 - y).abs().max().item())
    assert torch.equal(r2, r), (knob, (r2 - r).abs().max().item())


def test_grid_cap(cuda, monkeypatch):
    """MSW_GRID_CAP at F = 50: the grid-stride hop and edge-hop kernels make >= 3 iterations
    with a ragged last round, bit for bit the default schedule."""
    _clean_env(monkeypatch)
    build, cfg = msgnn_case(3, 50, [1, 3, 5])
    g = wet_state(make_multiscale_mesh(**mesh_config("small3"), T=T), seed=4)
    y, r, sched, _ = _run(build(), g, cuda)
    assert all(s["iters"] <= 1 for s in sched)
    for k, v in {"MSW_GRID_CAP": "2", "MSW_COOP_WAVES": "0", "MSW_HOP_ROWS": "0", "MSW_HOP_SPLIT": "0"}.items():
        monkeypatch.setenv(k, v)
    y2, r2, sched2, _ = _run(build(), g, cuda)
    for kind in ("hop", "edge_hop"):
        hits = [s for s in sched2 if s["kind"] == kind and s["iters"] >= 3 and s["ragged"]]
        assert hits and all(s["grid"] <= 2 and s["nt"] == 4 and " loop" in s["variant"] for s in hits), \
            (kind, [(s["variant"], s["scale"], s["grid"], s["iters"], s["ragged"]) for s in sched2])
    assert torch.equal(y2, y) and torch.equal(r2, r)
    P = state_dict_of(build())
    e, _ = assert_rollout_parity(r, orc.rollout(P, cfg(), g, T), P, cfg(), g, T, label="F50 K135 small3")
    WORST["F50 K135 small3"] = e


# ------------------------------------------------------------------ 6. fallback visibility
def test_auto_fallback_warns_once(cuda, monkeypatch):
    _clean_env(monkeypatch)
    g = _mesh(4).to(cuda)
    m = build_msgnn(4, 24, 2).to(cuda)
    assert m.engine == "auto" and m.engine_fallback_reason is None
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with torch.no_grad():
            m(g)
            m(g)
            m.rollout(g, 2)
    hits = [x for x in w if "HIP engine refused" in str(x.message)]
    assert len(hits) == 1, [str(x.message) for x in w]
    assert "hid_features" in str(hits[0].message)
    assert m.engine_fallback_reason and "hid_features" in m.engine_fallback_reason
    # asked for: no warning, no reason
    t = build_msgnn(4, 24, 2).to(cuda)
    t.engine = "torch"
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with torch.no_grad():
            t(g)
    assert not [x for x in w if "HIP engine refused" in str(x.message)] and t.engine_fallback_reason is None


def test_auto_runs_f50_on_the_engine(cuda, monkeypatch):
    _clean_env(monkeypatch)
    g = _mesh(4).to(cuda)
    m = build_msgnn(4, 50, 2).to(cuda)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with torch.no_grad():
            m(g)
            r = m.rollout(g, T)
    assert not [x for x in w if "HIP engine refused" in str(x.message)], [str(x.message) for x in w]
    assert m.engine_fallback_reason is None
    st = plan_for(m, g).stats()
    assert st["rollout_steps"] >= T and st["forward_calls"] >= 1 and st["padded_features"] == 64
    assert r.shape == (g.x.shape[0], 2, T)


# ------------------------------------------------------------------ 7. training at F = 50
TRAIN_TOL = 1e-4


def _close(ours, ref, r64_of):
    """tests/test_gpu_train_fuzz.py's rule: 1e-4 relative per tensor against torch's fp32
    autograd, or no further from a float64 autograd than torch's fp32 result is (x2, + 1e-5)."""
    assert ours.keys() == ref.keys()
    bad = {k: rel_err(ours[k], ref[k]) for k in ref if not rel_err(ours[k], ref[k]) <= TRAIN_TOL}
    if bad:
        r64 = r64_of()
        for k in list(bad):
            e_ours, e_ref = rel_err(ours[k], r64[k]), rel_err(ref[k], r64[k])
            if e_ours <= 2 * e_ref + 1e-5:
                del bad[k]
            else:
                bad[k] = (bad[k], e_ours, e_ref)
    assert not bad, bad


def _layer_grads(layer, x_s, x_d, ei, ea, wout, engine):
    layer.train_engine = engine
    layer.zero_grad(set_to_none=True)
    xs = x_s.clone().requires_grad_(True)
    xd = x_d.clone().requires_grad_(True)
    e = ea.clone().requires_grad_(True) if ea is not None else None
    out = layer(xs, xd, ei, e)
    (out * wout).sum().backward()
    g = {"out": out.detach(), "x_s": xs.grad, "x_d": xd.grad}
    if e is not None:
        g["edge_attr"] = e.grad
    for n, p in layer.named_parameters():
        g[n] = p.grad
    layer.train_engine = "auto"
    return g


@pytest.mark.parametrize("kind", ["processor", "intra"])
def test_training_layer_at_f50(cuda, kind):
    """One SWEGNN processor call (K = 2, edge features) and one intra-scale layer (K = 1, no
    filter, no gradient term, no edge features) at F = 50 on the HIP training kernels."""
    from models.gnn import SWEGNN
    from mswegnn import autograd as ag
    F = 50
    g = make_multiscale_mesh(n_coarse=2, num_scales=3, seed=7, T=2)
    ei = g.edge_index[:, g.edge_ptr[0]:g.edge_ptr[1]].to(cuda)
    N = g.num_nodes
    gen = torch.Generator().manual_seed(7)
    x_s, x_d = torch.randn(N, F, generator=gen), torch.randn(N, F, generator=gen)
    x_d[torch.rand(N, generator=gen) < 0.3] = 0.0
    wout = torch.randn(N, F, generator=gen)
    torch.manual_seed(7)
    if kind == "processor":
        ea = torch.randn(ei.shape[1], F, generator=gen)
        layer = SWEGNN(F, F, F, K=2, n_layers=3, activation="prelu")
    else:
        ea = None
        layer = SWEGNN(F, F, 0, K=1, normalize=True, with_filter_matrix=False, with_gradient=False, n_layers=3,
                       activation="prelu")
    dev = lambda t: t.to(cuda) if t is not None else None  # noqa: E731
    lay = copy.deepcopy(layer).to(cuda)
    assert ag.supported(lay, dev(x_s), dev(x_d), dev(ea))
    calls = ag.SWEGNN_CALLS[0]
    ours = _layer_grads(lay, dev(x_s), dev(x_d), ei, dev(ea), dev(wout), "auto")
    assert ag.SWEGNN_CALLS[0] > calls, "the HIP training kernels did not run"
    ref = _layer_grads(lay, dev(x_s), dev(x_d), ei, dev(ea), dev(wout), "torch")

    def r64():
        l64 = copy.deepcopy(layer).double().to(cuda)
        d64 = lambda t: t.double().to(cuda) if t is not None else None  # noqa: E731
        return _layer_grads(l64, d64(x_s), d64(x_d), ei, d64(ea), d64(wout), "torch")

    _close(ours, ref, r64)


def _model_grads(m, g, engine):
    m.engine = engine
    m.zero_grad(set_to_none=True)
    y = m(g)
    (y ** 2).mean().backward()
    out = {"y": y.detach()}
    out.update({n: p.grad for n, p in m.named_parameters()})
    return out


def test_training_whole_model_at_f50(cuda):
    from mswegnn import autograd as ag
    g = _mesh(4)
    m = build_msgnn(4, 50, 2)
    md = copy.deepcopy(m).to(cuda)
    sw, ml = ag.SWEGNN_CALLS[0], ag.MLP_CALLS[0]
    ours = _model_grads(md, g.to(cuda), "auto")
    assert ag.SWEGNN_CALLS[0] > sw and ag.MLP_CALLS[0] > ml, "the HIP training kernels did not run"
    ref = _model_grads(md, g.to(cuda), "torch")

    def r64():
        g64 = g.clone()
        for k in ("x", "edge_attr", "BC"):
            setattr(g64, k, getattr(g, k).double())
        return _model_grads(copy.deepcopy(m).double().to(cuda), g64.to(cuda), "torch")

    _close(ours, ref, r64)
    assert all(v is not None for v in ours.values())


def test_report_worst_error():
    """Prints the worst error against the oracle over the padded-width cases run above."""
    if not WORST:
        pytest.skip("needs the parity cases of this module to have run first")
    k = max(WORST, key=WORST.get)
    print(f"padded widths: worst rel error vs the oracle {WORST[k]:.2e} ({k}) over {len(WORST)} cases")
