"""The HIP engine on irregular, renumbered meshes (mswegnn.mesh.irregularize) against the
reference's fixtures and the oracle.

Every other GPU test draws its meshes from make_multiscale_mesh, an exact 1->4 quadtree in
hierarchical order.  The reference's real meshes are not (database/graph_creation.py:422-436,
498-518, 922-927), and the engine has code only they reach: children beyond the inline pooling
record and childless coarse rows with their "safe row" re-reads (in the fused pooling's slot
records and in k_pool_edge -- the row-layout k_pool is chosen only when a level's pooling tiles
do not fit resident, far above these sizes; tests/test_gpu_gridstride.py runs it on these meshes
under MSW_GRID_CAP), fine rows
without a parent in the fused unpooling, the dropped fused unpooling of a level with a two-parent node, in-degree 0/1/2
rows inside edge tiles, pack_order on an irregular degree sequence, orphans in a decomposition,
and the training kernels' pooling / intra-scale CSRs.  tests/test_irregular_mesh.py holds the
CPU side (the generator, and that these meshes have all of that for the seeds used here).
"""
import copy

import numpy as np
import pytest
import torch

from conftest import (REL_TOL, assert_rollout_parity, build_gnn, build_msgnn, manifest, per_step_rel, rel_err,
                      state_dict_of, weights)
import msgnn_torch as orc
from mswegnn.batch import collate
from mswegnn.mesh import irregularize, make_multiscale_mesh, make_single_scale_mesh, mesh_config, wet_state
from mswegnn.rollout import rollout_test
from test_gpu_schedule_fuzz import KNOB_VALUES
from test_irregular_mesh import GPU_SEEDS, back, irregular
from test_oracle_golden import IRREGULAR, irregular_fixture

pytestmark = pytest.mark.gpu

T = 6


def _hip(model, dev):
    model = model.to(dev)
    model.engine = "hip"
    return model


def _stats(model, g):
    from mswegnn.engine import plan_for
    return plan_for(model, g).stats()


def _clean_env(monkeypatch):
    for k in KNOB_VALUES:
        monkeypatch.delenv(k, raising=False)


def _native(model, g, forwards=0, steps=0):
    """The plan's own counters: the forward / rollout steps were the engine's launches."""
    st = _stats(model, g)
    assert st["forward_calls"] >= forwards and st["rollout_steps"] >= steps and st["kernels_per_step"] > 0, st
    return st


# ------------------------------------------------------------------ a. reference fixtures
@pytest.mark.parametrize("name", IRREGULAR)
def test_reference_fixture(cuda, name, monkeypatch):
    """HIP against the REFERENCE's own forward / rollout_test on irregular meshes (K4_F32;
    oracle/gen_golden_irregular.py): 1e-4 relative per step."""
    _clean_env(monkeypatch)
    g, fx = irregular_fixture(name)
    m = _hip(build_msgnn(4, 32, 4, state=weights("K4_F32")), cuda)
    gd = g.to(cuda)
    if "y" in fx:
        with torch.no_grad():
            e = rel_err(m(gd).cpu(), fx["y"])
        _native(m, gd, forwards=1)
    else:
        ref = torch.from_numpy(fx["rollout"])
        e = per_step_rel(m.rollout(gd).cpu(), ref)
        _native(m, gd, steps=ref.shape[-1])
    print(f"{name}: HIP vs reference, worst per-step rel {e:.2e}")
    assert e <= REL_TOL, (name, e)


# ------------------------------------------------------------------ b. the model family
def _family(case):
    """-> (model builder, oracle cfg, quadtree mesh) of one row of the model family."""
    if case == "S4_F32_K4":
        return (lambda: build_msgnn(4, 32, 4, state=weights("K4_F32")), manifest()["weights_K4_F32_cfg"],
                make_multiscale_mesh(**mesh_config("small"), T=T))
    if case == "S4_F16_K2":
        return (lambda: build_msgnn(4, 16, 2, state=weights("K2_F16")), manifest()["weights_K2_F16_cfg"],
                make_multiscale_mesh(**mesh_config("small"), T=T))
    if case == "S3_F64_K135":
        return (lambda: build_msgnn(3, 64, [1, 3, 5]), orc.msgnn_config(num_scales=3, hid_features=64, K=[1, 3, 5]),
                make_multiscale_mesh(**mesh_config("small3"), T=T))
    if case == "S2_F32_K5_noskip":
        return (lambda: build_msgnn(2, 32, 5, skip_connections=False),
                orc.msgnn_config(num_scales=2, hid_features=32, K=5, skip_connections=False),
                make_multiscale_mesh(n_coarse=12, num_scales=2, T=T))  # N0 = 1,153
    assert case == "S1_GNN"
    return (lambda: build_gnn(state=weights("gnn_F32_seed42")), manifest()["weights_gnn_F32_seed42_cfg"],
            make_single_scale_mesh(n_coarse=3, refinements=3, T=T))


FAMILY = ["S4_F32_K4", "S4_F16_K2", "S3_F64_K135", "S2_F32_K5_noskip", "S1_GNN"]


@pytest.mark.parametrize("wet", ["patch", "all_wet"])
@pytest.mark.parametrize("case", FAMILY)
def test_model_family_vs_oracle(cuda, case, wet, monkeypatch):
    """Forward + 6-step rollout against the oracle across the model family (incl. K = 5 hops),
    from a wet patch and from an all-wet state (no special row hides behind zeros)."""
    _clean_env(monkeypatch)
    build, cfg, g0 = _family(case)
    seed = GPU_SEEDS[FAMILY.index(case) % len(GPU_SEEDS)]
    g = irregularize(wet_state(g0, seed=seed, all_wet=(wet == "all_wet")), seed)[0]
    m = build()
    P = state_dict_of(m)
    ref_y, ref = orc.forward(P, cfg, g), orc.rollout(P, cfg, g, T)
    assert ref.abs().max() > 0.1
    mh = _hip(m, cuda)
    gd = g.to(cuda)
    with torch.no_grad():
        ey = rel_err(mh(gd).cpu(), ref_y)
    r = mh.rollout(gd, T).cpu()
    _native(mh, gd, forwards=1, steps=T)
    e, e_ref = assert_rollout_parity(r, ref, P, cfg, g, T, label=f"{case} {wet}")
    print(f"{case} {wet}: forward rel {ey:.2e}, rollout per-step rel {e:.2e}"
          + (f" (fp32 reference vs fp64 {e_ref:.2e})" if e_ref else ""))
    assert ey <= REL_TOL, (case, wet, ey)


# ------------------------------------------------------------------ c. batches
def test_batch_irregular_regular_irregular(cuda, monkeypatch):
    _clean_env(monkeypatch)
    gs = [irregular("small", GPU_SEEDS[0], wet=10, T=T)[0],
          wet_state(make_multiscale_mesh(**mesh_config("tiny"), seed=11, T=T), seed=11),
          irregular("tiny", GPU_SEEDS[1], wet=12, T=T)[0]]
    P, cfg = weights("K4_F32"), manifest()["weights_K4_F32_cfg"]
    m = _hip(build_msgnn(4, 32, 4, state=P), cuda)
    from mswegnn.rollout import adapt_batch_training
    batch = collate(gs).to(cuda)
    r = rollout_test(m, batch).cpu()
    assert r.shape == (sum(g.num_nodes for g in gs), 2, T)
    _native(m, adapt_batch_training(batch), steps=T)  # the batch's own plan (found by content) stepped T times
    a = 0
    for i, g in enumerate(gs):
        e, _ = assert_rollout_parity(r[a:a + g.num_nodes], orc.rollout(P, cfg, g, T), P, cfg, g, T, label=f"member {i}")
        print(f"batch member {i}: per-step rel {e:.2e}")
        a += g.num_nodes


# ------------------------------------------------------------------ d. relabelling is exact
@pytest.mark.parametrize("knob", [None, "MSW_TILE_PACK=0", "MSW_HOP_ROWS=2", "MSW_POOL_FUSE=0", "MSW_UNPOOL_FUSE=0",
                                  "MSW_COOP_WAVES=0"])
@pytest.mark.parametrize("F", [32, 64])
def test_relabelling_is_exact(cuda, F, knob, monkeypatch):
    """tiling.h: "results do not depend on the order" of the destinations.  order="kept" with
    permuted ids changes every row's number, tile and neighbours in the tile, but no sum's terms
    or their order: the rollout mapped back must be the unpermuted mesh's rollout BIT FOR BIT,
    under the default schedule and with each schedule switch that moves rows between kernels."""
    _clean_env(monkeypatch)
    if knob:
        monkeypatch.setenv(*knob.split("="))
    seed = GPU_SEEDS[2]
    ga, oa, g0 = irregular("small", seed, wet=seed, T=T, permute=False, order="kept")
    gb, ob, _ = irregular("small", seed, wet=seed, T=T, permute=True, order="kept")
    outs = []
    for g, old in ((ga, oa), (gb, ob)):
        m = _hip(build_msgnn(4, F, 4, state=weights("K4_F32") if F == 32 else None), cuda)
        gd = g.to(cuda)
        with torch.no_grad():
            y = m(gd).cpu()
        r = m.rollout(gd, T).cpu()
        _native(m, gd, forwards=1, steps=T)
        outs.append((back(y, old, g0.num_nodes), back(r, old, g0.num_nodes)))
    assert outs[0][1].abs().max() > 0.1
    for what, a, b in zip(("forward", "rollout"), outs[0], outs[1]):
        d = (a - b).abs()
        assert torch.equal(a, b), (f"{what} depends on the labelling (F {F}, {knob}): max |diff| {d.max().item():.3e} "
                                   f"on {int((d.flatten(1).sum(1) > 0).sum())} rows")


# ------------------------------------------------------------------ e. schedule variants
_default = {}


def _pair():
    return [irregular("small", GPU_SEEDS[3], wet=GPU_SEEDS[3], T=T)[0],
            wet_state(make_multiscale_mesh(**mesh_config("tiny"), seed=5, T=T), seed=5)]


def _sched_run(F, cuda):
    gs = _pair()
    m = _hip(build_msgnn(4, F, 4, state=weights("K4_F32") if F == 32 else None), cuda)
    g = gs[0].to(cuda)
    with torch.no_grad():
        y = m(g).cpu()
    out = (y, m.rollout(g, T).cpu(), rollout_test(m, collate(gs).to(cuda)).cpu())
    return out, _native(m, g, forwards=1, steps=T)["kernels_per_step"]


def _default_schedule(F, cuda, monkeypatch):
    _clean_env(monkeypatch)
    if F not in _default:
        _default[F] = _sched_run(F, cuda)
    return _default[F]


def _combos(n, base):
    names = sorted(KNOB_VALUES)
    out = []
    for i in range(n):
        rng = np.random.default_rng(base + i)
        pick = rng.choice(len(names), size=int(rng.integers(2, 7)), replace=False)
        out.append({names[k]: str(rng.choice(KNOB_VALUES[names[k]])) for k in sorted(pick)})
    return out


def _assert_same_as_default(F, cuda, monkeypatch, knobs):
    base, kps = _default_schedule(F, cuda, monkeypatch)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    flipped, kps_flipped = _sched_run(F, cuda)
    for what, a, b in zip(("forward", "rollout", "rollout_test batch"), flipped, base):
        assert a.shape == b.shape
        assert torch.equal(a, b), f"{what} differs under {knobs} at F {F}: {(a - b).abs().max().item():.3e}"
    return kps, kps_flipped


@pytest.mark.parametrize("F", [32, 64])
def test_default_schedule_vs_oracle(cuda, F, monkeypatch):
    """What every schedule variant below is compared with, against the oracle once."""
    base, _ = _default_schedule(F, cuda, monkeypatch)
    g = _pair()[0]
    m = build_msgnn(4, F, 4, state=weights("K4_F32") if F == 32 else None)
    P, cfg = state_dict_of(m), orc.msgnn_config(num_scales=4, hid_features=F, K=4)
    assert rel_err(base[0], orc.forward(P, cfg, g)) <= REL_TOL
    assert_rollout_parity(base[1], orc.rollout(P, cfg, g, T), P, cfg, g, T, label=f"default schedule F {F}")


@pytest.mark.parametrize("knob", sorted(KNOB_VALUES))
def test_each_switch_alone_is_bit_identical(cuda, knob, monkeypatch):
    for v in KNOB_VALUES[knob]:
        kps, kps_flipped = _assert_same_as_default(32, cuda, monkeypatch, {knob: v})
        if (knob, v) in (("MSW_POOL_FUSE", "0"), ("MSW_UNPOOL_FUSE", "0")):
            assert kps_flipped > kps, (knob, kps, kps_flipped)  # the switch took effect: launches came back


@pytest.mark.parametrize("F,i", [(32, i) for i in range(8)] + [(64, i) for i in range(4)])
def test_switch_combinations_are_bit_identical(cuda, F, i, monkeypatch):
    _assert_same_as_default(F, cuda, monkeypatch, _combos(8, 40_000 + F)[i])


# ------------------------------------------------------------------ f. single structures
def _run_structure(cuda, g, F=32):
    m = _hip(build_msgnn(4, F, 4, state=weights("K4_F32")), cuda)
    gd = g.to(cuda)
    with torch.no_grad():
        y = m(gd).cpu()
    r = m.rollout(gd, T).cpu()
    return y, r, _native(m, gd, forwards=1, steps=T)["kernels_per_step"]


@pytest.mark.parametrize("extra", ["childless", "children16", "isolated", "ghost_first"])
def test_single_structure(cuda, extra, monkeypatch):
    """One named structure each (a coarse face without children / with 16, a finest face without
    edges, the BC ghost as row 0 of its scale): against the oracle, and bit-identical with the
    pooling and the unpooling fused into the edge launches or launched on their own."""
    _clean_env(monkeypatch)
    g = irregular("small", GPU_SEEDS[0], wet=20, T=T, extra=(extra,))[0]
    P, cfg = weights("K4_F32"), manifest()["weights_K4_F32_cfg"]
    y, r, _ = _run_structure(cuda, g)
    ey = rel_err(y, orc.forward(P, cfg, g))
    e, _ = assert_rollout_parity(r, orc.rollout(P, cfg, g, T), P, cfg, g, T, label=extra)
    print(f"{extra}: forward rel {ey:.2e}, rollout per-step rel {e:.2e}")
    assert ey <= REL_TOL
    kps = {}
    for pf in ("0", "1"):
        for uf in ("0", "1"):
            monkeypatch.setenv("MSW_POOL_FUSE", pf)
            monkeypatch.setenv("MSW_UNPOOL_FUSE", uf)
            y2, r2, kps[pf, uf] = _run_structure(cuda, g)
            assert torch.equal(y2, y) and torch.equal(r2, r), (extra, pf, uf)
    assert kps["1", "1"] < kps["0", "1"] < kps["0", "0"] and kps["1", "1"] < kps["1", "0"], kps


def test_two_parents_brings_the_unpooling_launch_back(cuda, monkeypatch):
    """A fine face of level 1 with two parents: the fused unpooling holds one parent per slot
    side, so that level keeps its unpooling launch (one launch more per step than the same mesh
    without the second pair) -- also when MSW_UNPOOL_FUSE=1 asks for the fusion -- and the
    result matches the oracle, which sums both parents' messages."""
    _clean_env(monkeypatch)
    g = irregular("small", GPU_SEEDS[0], wet=20, T=T, extra=("two_parents",))[0]
    plain = irregular("small", GPU_SEEDS[0], wet=20, T=T)[0]
    assert g.intra_mesh_edge_index.shape[1] == plain.intra_mesh_edge_index.shape[1] + 1
    P, cfg = weights("K4_F32"), manifest()["weights_K4_F32_cfg"]
    y, r, kps = _run_structure(cuda, g)
    assert rel_err(y, orc.forward(P, cfg, g)) <= REL_TOL
    e, _ = assert_rollout_parity(r, orc.rollout(P, cfg, g, T), P, cfg, g, T, label="two_parents")
    print(f"two_parents: rollout per-step rel {e:.2e}")
    assert not torch.equal(orc.forward(P, cfg, g), orc.forward(P, cfg, plain))  # the second parent counts
    _, _, kps_plain = _run_structure(cuda, plain)
    assert kps > kps_plain, (kps, kps_plain)
    monkeypatch.setenv("MSW_UNPOOL_FUSE", "1")
    y1, r1, kps1 = _run_structure(cuda, g)
    assert torch.equal(y1, y) and torch.equal(r1, r) and kps1 > kps_plain


# ------------------------------------------------------------------ g. decomposition
@pytest.mark.parametrize("parts", [2, 3])
def test_decomposition_of_an_irregular_mesh(cuda, parts, monkeypatch):
    """PartitionedRollout (orphans owned by a neighbour's rank, families of 0..10 children, moved
    pairs): hipGraph replay and eager, both bit for bit the undivided rollout."""
    from mswegnn import _lib as L
    from mswegnn.partition import PartitionedRollout
    _clean_env(monkeypatch)
    g = irregular("small", GPU_SEEDS[1], wet=30, T=T)[0]
    P, cfg = weights("K4_F32"), manifest()["weights_K4_F32_cfg"]
    m = _hip(build_msgnn(4, 32, 4, state=P), cuda)
    gd = g.to(cuda)
    whole = m.rollout(gd, T).cpu()
    assert_rollout_parity(whole, orc.rollout(P, cfg, g, T), P, cfg, g, T, label=f"undivided ({parts} parts)")
    pr = PartitionedRollout(m, gd, parts, cuda)
    try:
        graphed = pr.rollout(gd.x, gd.BC, gd.node_BC, gd.type_BC, T).cpu()
        assert all(pl.stats()["rollout_steps"] >= T for pl in pr.plans)
        assert torch.equal(graphed, whole), (graphed - whole).abs().max().item()
        L.check(L.lib().msw_set_group_graph(pr.plans[0]._h, 0))
        eager = pr.rollout(gd.x, gd.BC, gd.node_BC, gd.type_BC, T).cpu()
        assert torch.equal(eager, whole), (eager - whole).abs().max().item()
    finally:
        pr.close()


# ------------------------------------------------------------------ h. training kernels
def _judge(ours, ref, exact, label):
    """tests/test_gpu_train.py's bar (1e-4 per tensor against torch's fp32 autograd); where fp32
    cannot resolve a tensor that finely, tests/test_gpu_train_fuzz.py's float64 arbiter: no
    further from a float64 autograd of the same computation than torch's fp32 result is
    (x2, plus 1e-5).  exact: () -> the float64 tensors.  Returns the worst error vs torch fp32."""
    from test_gpu_train import TOL
    assert ours.keys() == ref.keys()
    for k in ref:
        assert ours[k] is not None and ref[k] is not None, (label, k)
    errs = {k: rel_err(ours[k], ref[k]) for k in ref}
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    if bad:
        r64 = exact()
        for k in list(bad):
            e_ours, e_ref = rel_err(ours[k], r64[k]), rel_err(ref[k], r64[k])
            if e_ours <= 2 * e_ref + 1e-5:
                del bad[k]
            else:
                bad[k] = (bad[k], e_ours, e_ref)
    assert not bad, (label, bad)
    return max(errs.values())


def _train_mesh(cuda, extra=()):
    return irregular("tiny", GPU_SEEDS[0], wet=1, T=4, extra=extra)[0].to(cuda)


def test_training_step_gradients_on_an_irregular_mesh(cuda):
    """tests/test_gpu_train.py::test_msgnn_training_step_gradients on an irregular tiny mesh."""
    from mswegnn import autograd as ag
    g = _train_mesh(cuda)
    m = build_msgnn(4, 32, 4, state=weights("K4_F32")).to(cuda)
    m.train()
    tgt = torch.rand(g.num_nodes, 2, device=cuda, generator=torch.Generator(cuda).manual_seed(7))

    def step(model, graph, engine):
        model.zero_grad(set_to_none=True)
        model.engine = engine
        y = model(graph)
        ((y - tgt.to(y.dtype)) ** 2).mean().backward()
        return {"y": y.detach(), **{n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}}

    def exact():
        g64 = g.clone()
        for k in ("x", "edge_attr", "BC"):
            setattr(g64, k, getattr(g, k).double())
        return step(copy.deepcopy(m).double(), g64, "torch")
    ref = step(m, g, "torch")
    calls = ag.MLP_CALLS[0], ag.POOL_CALLS[0], ag.SWEGNN_CALLS[0]
    ours = step(m, g, "auto")
    assert ag.MLP_CALLS[0] > calls[0] and ag.POOL_CALLS[0] > calls[1] and ag.SWEGNN_CALLS[0] > calls[2]  # the HIP path ran
    e = _judge(ours, ref, exact, "MSGNN irregular")
    print(f"MSGNN on an irregular mesh: worst gradient rel err {e:.2e} over {len(ref)} tensors")


@pytest.mark.parametrize("extra", [(), ("childless",)])
def test_mean_pooling_gradients_on_an_irregular_mesh(cuda, extra):
    """tests/test_gpu_train.py::test_mean_pooling_gradients_vs_torch_autograd over every level of
    an irregular tiny mesh: 0..n children per coarse face, orphans (zero input gradient), and
    once more with a childless coarse face (zero output row)."""
    from mswegnn import autograd as ag
    from mswegnn.autograd import pool_apply
    g = _train_mesh(cuda, extra)
    m = build_msgnn(4, 32, 4, state=weights("K4_F32")).to(cuda)
    iei, iep, npt = g.intra_mesh_edge_index, g.intra_edge_ptr, g.node_ptr
    torch.manual_seed(2)
    x = torch.randn(g.num_nodes, 32, device=cuda)
    for i in range(3):
        pe = iei[:, iep[i]:iep[i + 1]]
        wout = torch.randn_like(x)
        cnt = torch.bincount(pe[0] - npt[i + 1], minlength=int(npt[i + 2] - npt[i + 1]))
        orphans = int(npt[i + 1] - npt[i]) - len(torch.unique(pe[1]))
        if i == 0:
            # the ghost's row is the last one; a face lost all its children only with "childless"
            assert int(cnt.max()) > 4 and orphans > 0 and int((cnt[:-1] == 0).sum()) == len(extra)

        def run(fn, dt=torch.float32):
            xx = x.detach().clone().to(dt).requires_grad_(True)  # a leaf of its own per run
            y = fn(xx)
            (y * wout.to(dt)).sum().backward()
            return {"y": y.detach(), "x": xx.grad}
        ref = run(lambda xx: m._pooling(xx, pe[1], pe[0], "mean", False))
        calls = ag.POOL_CALLS[0]
        ours = run(lambda xx: pool_apply(xx, pe))
        assert ag.POOL_CALLS[0] == calls + 1
        # two gradients of their own; a fine row gets one exactly when it has a parent
        assert ours["x"] is not ref["x"] and ours["x"].data_ptr() != ref["x"].data_ptr()
        child = torch.zeros(g.num_nodes, dtype=torch.bool, device=cuda)
        child[pe[1]] = True
        assert bool((ours["x"][child].abs().amax(1) > 0).all()) and not bool(ours["x"][~child].any())
        e = _judge(ours, ref, lambda: run(lambda xx: m._pooling(xx, pe[1], pe[0], "mean", False), torch.float64),
                   f"pool level {i} {extra}")
        print(f"pool level {i} {extra}: children {int(cnt.min())}..{int(cnt.max())}, {orphans} orphans, "
              f"worst rel err {e:.2e}")


def test_intra_scale_gradients_on_an_irregular_mesh(cuda):
    """The intra_scale_gnn part of tests/test_gpu_train.py::test_intra_scale_and_variant_gradients
    (K = 1, no edge features, no filter, s * out[row] messages over the (coarse, fine) pairs) on
    an irregular tiny mesh: fine rows with no in-edge, coarse rows with 0..n out-edges."""
    from mswegnn import autograd as ag
    from test_gpu_train import _encoded_inputs, _grads
    g = _train_mesh(cuda)
    m = build_msgnn(4, 32, 4, state=weights("K4_F32")).to(cuda)
    x_s, x_d, _, _ = _encoded_inputs(m, g, 0)
    wout = torch.randn(x_d.shape, device=cuda, generator=torch.Generator(cuda).manual_seed(5))
    worst = 0.0
    for level in range(3):
        iei = g.intra_mesh_edge_index[:, g.intra_edge_ptr[level]:g.intra_edge_ptr[level + 1]]
        layer = m.intra_scale_gnn[2 - level]
        calls = ag.SWEGNN_CALLS[0]
        ours = _grads(layer, x_s, x_d, iei, None, wout, "auto")
        assert ag.SWEGNN_CALLS[0] == calls + 1
        ref = _grads(layer, x_s, x_d, iei, None, wout, "torch")
        worst = max(worst, _judge(ours, ref, lambda: _grads(copy.deepcopy(layer).double(), x_s.double(), x_d.double(),
                                                            iei, None, wout.double(), "torch"), f"intra level {level}"))
    print(f"intra_scale_gnn on irregular levels: worst rel err {worst:.2e}")
