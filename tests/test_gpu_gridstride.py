"""Every grid-stride kernel of the large-mesh path, on small meshes, making several loop
iterations per wave (MSW_GRID_CAP, plan.h Knobs).

The large-mesh family (grid-stride k_encode, k_edge_hop<.., LOOP>, k_hop<.., LOOP>, k_hop_rows on
a capped grid, the row-layout k_pool, k_epi<.., LOOP>, the capped k_edge_mlp) is otherwise reached
only when a launch does not fit the chip in one round: at config 5's size, one width, a quadtree
mesh.  MSW_GRID_CAP=n clamps every residency figure of a plan to n workgroups, so a 1.5 k-node
plan gets the schedule of a mesh too large for an n-workgroup chip, and a wave walks 2, 3 or
28 tiles.  Each case here

  (a) reads from EnginePlan.schedule() -- printed by the code that picks what is launched --
      that the capped plan holds the kernel variant the case is named for, at the expected
      width, with the iteration count it asks for: "two" (iters == 2: the pipelined loops'
      prologue and drain only) or "many" (iters >= 3 with a ragged last round: the steady
      state's rotation too);
  (b) compares plan.forward, a 4-step plan.rollout from a wet state and a batched rollout_test
      over two meshes with the default schedule's: torch.equal, every variant is bit-identical;
  (c) relies on test_default_schedule_vs_oracle: the default schedule of the same (model, mesh)
      against the oracle at REL_TOL per step, so a capped plan cannot agree with a wrong default.

test_every_row_was_reached then checks that the cases together covered every row of ROWS at
every width its kernel exists for, in both iteration classes.

Shapes: mesh_config("small") (4 scales; 221 / 53 / 13 / 3 edge tiles, 73 / 19 / 5 / 2 row
tiles, 27 encoder chunks) and "small3" (its first three scales), caps 1-3 -- and 13 / 14 for
the encoder's "two" class, whose 26 / 27 chunks no cap of 1-3 walks in two rounds.  The
iteration counts in CASES were read from plan.schedule() on an MI355X.

Not here: a coarse face with 17 children ("children17"), which plan creation rejects by
contract (tests/test_host_sanitizer.py); the irregular meshes carry "children16" instead, and
faces of 5-10 children, which take the same child walk beyond the inline pooling record.
MSW_EPI_SPLIT_TILES=1 (not 0, which switches the row epilogue off) selects k_epi on every scale.
"""
import copy
import os

import pytest
import torch

from conftest import REL_TOL, assert_rollout_parity, build_gnn, build_msgnn, manifest, rel_err, state_dict_of, weights
import msgnn_torch as orc
from mswegnn.batch import collate
from mswegnn.engine import EnginePlan, plan_for
from mswegnn.mesh import make_multiscale_mesh, make_single_scale_mesh, mesh_config, wet_state
from mswegnn.rollout import adapt_batch_training, rollout_test
from test_irregular_mesh import GPU_SEEDS, irregular

pytestmark = pytest.mark.gpu

T = 4
EXTRA = ("childless", "children16", "two_parents", "isolated")

# model -> (builder, oracle config, width)
MODELS = {
    "K4_F32": (lambda: build_msgnn(4, 32, 4, state=weights("K4_F32")), lambda: manifest()["weights_K4_F32_cfg"], 32),
    "K2_F16": (lambda: build_msgnn(4, 16, 2, state=weights("K2_F16")), lambda: manifest()["weights_K2_F16_cfg"], 16),
    # K2_F16 has no middle hop: a seeded F = 16 model with K = 3 for rows 5 and 7
    "K3_F16": (lambda: build_msgnn(3, 16, 3), lambda: orc.msgnn_config(num_scales=3, hid_features=16, K=3), 16),
    # K = 1 on the finest scale: its processors' only hop is k_edge_hop<.., 1> (row 4)
    "K135_F64": (lambda: build_msgnn(3, 64, [1, 3, 5]),
                 lambda: orc.msgnn_config(num_scales=3, hid_features=64, K=[1, 3, 5]), 64),
    # no PReLU: the ACT = -1 instantiations
    "relu_F32": (lambda: build_msgnn(3, 32, [1, 2, 3], mlp_activation="relu", gnn_activation="tanh"),
                 lambda: orc.msgnn_config(num_scales=3, hid_features=32, K=[1, 2, 3], mlp_activation="relu",
                                          gnn_activation="tanh"), 32),
    "GNN": (lambda: build_gnn(state=weights("gnn_F32_seed42")), lambda: manifest()["weights_gnn_F32_seed42_cfg"], 32),
}


def _mesh(key):
    """-> [the case's mesh, a second mesh for the batch]: wet patches, or an all-wet state."""
    if key == "single":
        return [wet_state(make_single_scale_mesh(n_coarse=3, refinements=3, T=T), seed=4),
                wet_state(make_single_scale_mesh(n_coarse=2, refinements=2, seed=5, T=T), seed=5)]
    if key == "irrA":    # ids kept
        g, tiny = irregular("small", GPU_SEEDS[0], wet=4, T=T, extra=EXTRA, permute=False)[0], "tiny"
    elif key == "irrB":  # ids permuted, three scales
        g, tiny = irregular("small3", GPU_SEEDS[1], wet=4, T=T, extra=EXTRA, permute=True)[0], None
    else:
        name, _, wet = key.partition("/")
        g = wet_state(make_multiscale_mesh(**mesh_config(name), T=T), seed=4, all_wet=(wet == "allwet"))
        tiny = "tiny" if name == "small" else None
    second = (make_multiscale_mesh(**mesh_config(tiny), seed=5, T=T) if tiny else
              make_multiscale_mesh(n_coarse=3, num_scales=3, seed=5, T=T))
    return [g, wet_state(second, seed=5)]


# row of the issue's table -> (kernel variant as plan.schedule() names it, the switches that
# select it on a small mesh besides the cap)
ROWS = {
    1: ("encode loop stream", {"MSW_DEFER_DECODE": "0", "MSW_ENC_COOP": "0"}),
    2: ("encode loop dec", {"MSW_DEFER_DECODE": "1", "MSW_ENC_COOP": "0"}),
    3: ("edge_hop loop first", {"MSW_COOP_WAVES": "0"}),
    4: ("edge_hop loop last", {"MSW_COOP_WAVES": "0", "MSW_UNPOOL_FUSE": "0"}),
    5: ("hop loop mid", {"MSW_HOP_ROWS": "0", "MSW_HOP_SPLIT": "0"}),
    6: ("hop loop last", {"MSW_COOP_WAVES": "0", "MSW_EPI_SPLIT_TILES": "100000"}),
    7: ("hop rows", {"MSW_HOP_ROWS": "2"}),
    8: ("pool rows loop", {"MSW_POOL_FUSE": "0", "MSW_COOP_WAVES": "0"}),
    9: ("epi loop", {"MSW_EPI_SPLIT_TILES": "1"}),
    10: ("edge_mlp", {"MSW_SPLIT_EDGE_MLP": "1"}),
}
WIDTHS = {r: ((64,) if r == 10 else (16, 32, 64)) for r in ROWS}
POOL_ROWS_FIT = "pool rows"  # row 8's other kernel, k_pool<NT, false>: the row tiles fit the cap

# (row, model, mesh, cap, want): want = "two" (a launch of the variant with iters == 2), "many"
# (iters >= 3, ragged), "both", or "loop" (iters >= 2: the irregular meshes, whose classes the
# regular ones cover); "+fit": the capped plan also holds POOL_ROWS_FIT
CASES = [
    (1, "K4_F32", "small", 2, "many"), (1, "K4_F32", "small", 14, "two"),
    (1, "K2_F16", "small/allwet", 2, "many"), (1, "K2_F16", "small/allwet", 14, "two"),
    (1, "K135_F64", "small3", 3, "many"), (1, "K135_F64", "small3", 13, "two"),
    (1, "relu_F32", "small3", 3, "many"),
    (2, "K4_F32", "small", 2, "many"), (2, "K4_F32", "small", 14, "two"),
    (2, "K2_F16", "small/allwet", 2, "many"), (2, "K2_F16", "small/allwet", 14, "two"),
    (2, "K135_F64", "small3", 3, "many"), (2, "K135_F64", "small3", 13, "two"),
    (2, "GNN", "single", 2, "many"),
    (3, "K4_F32", "small", 2, "both"), (3, "K2_F16", "small/allwet", 2, "both"), (3, "K135_F64", "small3", 2, "both"),
    (3, "relu_F32", "small3", 1, "many"), (3, "GNN", "single", 2, "many"),
    (3, "K4_F32", "irrA", 2, "loop"), (3, "K135_F64", "irrB", 2, "loop"),
    (4, "K4_F32", "small", 1, "both"), (4, "K2_F16", "small/allwet", 1, "both"), (4, "K135_F64", "small3", 3, "both"),
    (4, "relu_F32", "small3", 1, "both"),
    (4, "K4_F32", "irrA", 1, "loop"), (4, "K135_F64", "irrB", 3, "loop"),
    (5, "K4_F32", "small", 1, "both"), (5, "K3_F16", "small3/allwet", 1, "both"), (5, "K135_F64", "small3", 2, "both"),
    (5, "K4_F32", "irrA", 1, "loop"), (5, "K135_F64", "irrB", 2, "loop"),
    (6, "K4_F32", "small", 1, "both"), (6, "K2_F16", "small/allwet", 1, "both"), (6, "K135_F64", "small3", 2, "both"),
    (6, "relu_F32", "small3", 1, "both"), (6, "GNN", "single", 2, "many"),
    (6, "K4_F32", "irrA", 1, "loop"), (6, "K135_F64", "irrB", 2, "loop"),
    (7, "K4_F32", "small", 2, "both"), (7, "K3_F16", "small3/allwet", 2, "both"),
    (7, "K135_F64", "small3", 1, "many"), (7, "K135_F64", "small3", 2, "two"),
    (7, "K4_F32", "irrA", 2, "loop"), (7, "K135_F64", "irrB", 1, "loop"),
    (8, "K4_F32", "small", 1, "many"), (8, "K4_F32", "small", 2, "two+fit"),
    (8, "K2_F16", "small/allwet", 1, "many"), (8, "K2_F16", "small/allwet", 2, "two+fit"),
    (8, "K135_F64", "small3", 1, "both"), (8, "K135_F64", "small3", 3, "two+fit"),
    (8, "K4_F32", "irrA", 1, "loop"), (8, "K135_F64", "irrB", 1, "loop"),
    (9, "K4_F32", "small", 1, "many"), (9, "K4_F32", "small", 2, "two"),
    (9, "K2_F16", "small/allwet", 1, "many"), (9, "K2_F16", "small/allwet", 2, "two"),
    (9, "K135_F64", "small3", 1, "both"), (9, "relu_F32", "small3", 1, "many"), (9, "GNN", "single", 1, "many"),
    (9, "K4_F32", "irrA", 1, "loop"), (9, "K135_F64", "irrB", 1, "loop"),
    (10, "K135_F64", "small3", 1, "both"), (10, "K135_F64", "small3/allwet", 2, "many"),
]
PAIRS = sorted({(m, g) for _, m, g, _, _ in CASES})

_seen = set()     # (row or "8 fit", width, "two" / "many") asserted by a case that passed
_ran = []         # cases started
_defaults = {}    # (model, mesh) -> the default schedule's results
_meshes = {}


def _clean_env(monkeypatch):
    for k in [k for k in os.environ if k.startswith("MSW_")]:
        monkeypatch.delenv(k)


def _graphs(key):
    if key not in _meshes:
        _meshes[key] = _mesh(key)
    return _meshes[key]


def _run(model_key, mesh_key, cuda):
    """-> (forward, rollout, batched rollout_test, rollout schedule, the batch plan's schedule)
    under the MSW_* variables set now: fresh plans and a fresh model (plan_for caches per model)."""
    gs = _graphs(mesh_key)
    m = MODELS[model_key][0]().to(cuda)
    g = gs[0].to(cuda)
    plan = EnginePlan(m, g, cuda)
    try:
        sched = plan.schedule()
        y = plan.forward(g.x).cpu()
        r = plan.rollout(g.x, g.BC, g.node_BC, g.type_BC, T).cpu()
        assert plan.stats()["rollout_steps"] >= T and plan.stats()["kernels_per_step"] == len(sched)
    finally:
        plan.close()
    mb = copy.deepcopy(m)
    mb.engine = "hip"
    batch = collate(gs).to(cuda)
    rb = rollout_test(mb, batch).cpu()
    bplan = plan_for(mb, adapt_batch_training(batch))
    assert bplan.stats()["rollout_steps"] >= T
    return y, r, rb, sched, bplan.schedule()


def _default(model_key, mesh_key, cuda, monkeypatch):
    _clean_env(monkeypatch)
    if (model_key, mesh_key) not in _defaults:
        _defaults[model_key, mesh_key] = _run(model_key, mesh_key, cuda)
    return _defaults[model_key, mesh_key]


def _classes(sched, variant, nt):
    hits = [s for s in sched if s["variant"] == variant and s["nt"] == nt]
    cls = set()
    for s in hits:
        assert 0 < s["grid"] and s["iters"] == -(-s["units"] // (s["grid"] * s["per_wg"])), s
        if s["iters"] == 2:
            cls.add("two")
        if s["iters"] >= 3 and s["ragged"]:
            cls.add("many")
        if s["iters"] >= 2:
            cls.add("loop")
    return hits, cls


@pytest.mark.parametrize("model_key,mesh_key", PAIRS)
def test_default_schedule_vs_oracle(cuda, model_key, mesh_key, monkeypatch):
    """(c) What the capped plans are compared with, against the oracle once per (model, mesh):
    forward and the 4-step rollout at REL_TOL per step.  No launch of a default plan loops."""
    y, r, _, sched, _ = _default(model_key, mesh_key, cuda, monkeypatch)
    assert all(s["iters"] <= 1 and " loop" not in s["variant"] and s["variant"] != "hop rows" for s in sched), sched
    g = _graphs(mesh_key)[0]
    m = MODELS[model_key][0]()
    P, cfg = state_dict_of(m), MODELS[model_key][1]()
    ey = rel_err(y, orc.forward(P, cfg, g))
    ref = orc.rollout(P, cfg, g, T)
    assert ref.abs().max() > 0.1
    e, e_ref = assert_rollout_parity(r, ref, P, cfg, g, T, label=f"{model_key} {mesh_key}")
    print(f"{model_key} {mesh_key}: default schedule, forward rel {ey:.2e}, rollout per-step rel {e:.2e}"
          + (f" (fp32 reference vs fp64 {e_ref:.2e})" if e_ref else ""))
    assert ey <= REL_TOL, (model_key, mesh_key, ey)


@pytest.mark.parametrize("row,model_key,mesh_key,cap,want", CASES,
                         ids=[f"row{r}-{m}-{g.replace('/', '_')}-cap{c}-{w}" for r, m, g, c, w in CASES])
def test_grid_stride_kernel_under_the_cap(cuda, row, model_key, mesh_key, cap, want, monkeypatch):
    _ran.append((row, model_key, mesh_key, cap))
    base = _default(model_key, mesh_key, cuda, monkeypatch)
    variant, env = ROWS[row]
    F = MODELS[model_key][2]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("MSW_GRID_CAP", str(cap))
    y, r, rb, sched, bsched = _run(model_key, mesh_key, cuda)
    # (a) reach and iterations, from the plan's own description of what it launches
    want, _, fit = want.partition("+")
    hits, cls = _classes(sched, variant, F // 16)
    summary = [(s["variant"], s["scale"], s["grid"], s["iters"], s["ragged"]) for s in sched]
    assert hits, f"row {row}: no '{variant}' launch under {env} + cap {cap}: {summary}"
    assert all(s["grid"] <= cap for s in hits), hits
    need = {"both": {"two", "many"}}.get(want, {want})
    assert need <= cls, (f"row {row} '{variant}' F {F}: wanted {sorted(need)}, the plan has "
                         f"{[(s['scale'], s['iters'], s['ragged']) for s in hits]}")
    if row <= 2:  # the rollout's encoder; forward mode has no deferred decoder to run
        assert len(hits) == 1 and sched[0]["variant"] == variant
    if fit:
        assert _classes(sched, POOL_ROWS_FIT, F // 16)[0], summary
    assert any(s["iters"] >= 2 for s in bsched), "the batch's plan was not built under the cap"
    # (b) bit identity with the default schedule
    for what, a, b in zip(("forward", "rollout", "rollout_test batch"), (y, r, rb), base):
        assert a.shape == b.shape
        d = (a - b).abs()
        assert torch.equal(a, b), (f"{what} differs under '{variant}' (row {row}, {model_key}, {mesh_key}, cap {cap}): "
                                   f"max |diff| {d.max().item():.3e} on {int((d.flatten(1).sum(1) > 0).sum())} rows")
    for c in need & {"two", "many"}:
        _seen.add((row, F, c))
    if fit:
        _seen.add(("8 fit", F, "reached"))


def test_decomposition_under_the_cap(cuda, monkeypatch):
    """PartitionedRollout, 2 parts, every part's plan built under the cap: bit for bit the
    undivided default rollout.  A part's halo rows are the last rows of each scale's range --
    the ragged last round of its grid-stride launches."""
    from mswegnn.partition import PartitionedRollout
    whole = _default("K4_F32", "small", cuda, monkeypatch)[1]
    monkeypatch.setenv("MSW_GRID_CAP", "2")
    monkeypatch.setenv("MSW_COOP_WAVES", "0")
    g = _graphs("small")[0].to(cuda)
    m = MODELS["K4_F32"][0]().to(cuda)
    pr = PartitionedRollout(m, g, 2, cuda)
    try:
        for pl in pr.plans:
            sched = pl.schedule()
            for variant in ("edge_hop loop first", "hop rows", "hop loop last"):
                hits, cls = _classes(sched, variant, 2)
                assert hits and "loop" in cls, (variant, [(s["variant"], s["scale"], s["iters"]) for s in sched])
        out = pr.rollout(g.x, g.BC, g.node_BC, g.type_BC, T).cpu()
        assert all(pl.stats()["rollout_steps"] >= T for pl in pr.plans)
    finally:
        pr.close()
    assert torch.equal(out, whole), (out - whole).abs().max().item()


def test_every_row_was_reached():
    """Across the cases above, every row of ROWS ran at every width its kernel exists for, once
    with iters == 2 and once with iters >= 3 and a ragged last round; k_pool<NT, false> (row
    8's one-round variant) was reached at every width.  A row that no case reached fails."""
    if len(_ran) < len(CASES):
        pytest.skip("needs every case of this module to have run first")
    expected = {(row, F, c) for row in ROWS for F in WIDTHS[row] for c in ("two", "many")}
    expected |= {("8 fit", F, "reached") for F in (16, 32, 64)}
    missing = sorted(expected - _seen, key=str)
    assert not missing, f"not reached (row, F, class): {missing}"
