"""The locality order on the GPU: k_hilbert_keys and the radix sort against the numpy restatements of
tests/locality_cases.py bit for bit (outputs between canary words), mswegnn.locality.row_order
against its CPU path, and the engine: a plan built with a row order (msw_plan_create_ordered) gives
the bits of the plan built without one, in the caller's numbering, for every order, model width and
mesh kind; the plan cache tells graphs with and without an order apart; bad orders are refused.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import locality_cases as lc
import msgnn_torch as orc
from conftest import REL_TOL, build_gnn, build_msgnn, manifest, per_step_rel, rel_err, weights
from mswegnn import _lib
from mswegnn import locality as loc
from mswegnn.batch import collate
from mswegnn.engine import EnginePlan, plan_for
from mswegnn.mesh import Graph, irregularize, make_multiscale_mesh, make_single_scale_mesh, mesh_config, wet_state
from mswegnn.rollout import adapt_batch_training, apply_boundary_condition, use_prediction
from test_gpu_raster import PADS, Out, stream_ptr

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -3


# ----------------------------------------------------------------------------- keys
def raw_keys(xy, box, cuda, pad=37):
    d = torch.from_numpy(np.ascontiguousarray(xy, np.float64).reshape(-1, 2)).to(cuda)
    out = Out((d.shape[0],), cuda, pad)
    code = _lib.lib().msw_hilbert_keys(C.c_void_p(d.data_ptr()), d.shape[0], *[float(v) for v in box], out.ptr,
                                       stream_ptr())
    torch.cuda.synchronize()
    return code, out


@pytest.mark.parametrize("name", list(lc.KEY_CASES))
def test_keys(cuda, name):
    xy, box = lc.KEY_CASES[name]
    want = lc.hilbert_keys_ref(xy, box)
    for pad in PADS:
        code, out = raw_keys(xy, box, cuda, pad)
        assert code == 0
        out.check(want, name)
    got = loc.hilbert_keys(xy, box, device=cuda)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want.astype(np.int64))


def test_keys_counts(cuda):
    """n = 0, 1, 63, 64, 65, 129 and two and three grid-stride rounds (sizes from msw_locality_launch)."""
    grid, per_wg, _ = loc.locality_launch(2 ** 26)
    sizes = [0, 1, 63, 64, 65, 129, grid * per_wg + 1, 2 * grid * per_wg + 7]
    assert [loc.locality_launch(n)[2] for n in sizes[-2:]] == [2, 3]
    box = (-3.0, 2.0, 7.0)
    rng = np.random.default_rng(4)
    none = Out((1,), cuda)
    d = torch.zeros(1, 2, dtype=torch.float64, device=cuda)
    assert _lib.lib().msw_hilbert_keys(C.c_void_p(d.data_ptr()), 0, *box, none.ptr, stream_ptr()) == 0
    torch.cuda.synchronize()
    assert none.untouched()
    for n in sizes[1:]:
        xy = np.array(box[:2]) + rng.random((n, 2)) * box[2]
        code, out = raw_keys(xy, box, cuda)
        assert code == 0
        out.check(lc.hilbert_keys_ref(xy, box), f"n = {n}")


# ----------------------------------------------------------------------------- sort
def raw_sort(keys, cuda, seg_ptr=None, pad=37):
    keys = np.ascontiguousarray(keys, np.uint32)
    n = len(keys)
    d = torch.from_numpy(keys.view(np.int32).copy()).to(cuda) if n else torch.zeros(1, dtype=torch.int32, device=cuda)
    seg = np.ascontiguousarray([0, n] if seg_ptr is None else seg_ptr, np.int64)
    out = Out((max(n, 1),), cuda, pad)
    st = _lib.MswLocalityStats()
    code = _lib.lib().msw_locality_sort(C.c_void_p(d.data_ptr()), n, seg.ctypes.data_as(_lib.c_int64_p), len(seg) - 1,
                                        out.ptr, cuda.index or 0, stream_ptr(), C.byref(st))
    return code, out, st


def check_sort(keys, cuda, seg_ptr=None, label=""):
    code, out, st = raw_sort(keys, cuda, seg_ptr)
    assert code == 0, _lib.lib().msw_last_error()
    if len(keys) == 0:
        assert out.untouched()
        return st
    out.check(lc.order_ref(keys, seg_ptr).astype(np.int32), label)
    return st


@pytest.mark.parametrize("pattern", lc.SORT_PATTERNS)
def test_sort_patterns(cuda, pattern):
    for n in (1000, 5000):                      # 4 and 20 workgroups of one round
        keys = lc.sort_keys(pattern, n)
        check_sort(keys, cuda, label=f"{pattern} n = {n}")
        if pattern == "all_equal":              # stability gives the identity
            _, out, _ = raw_sort(keys, cuda)
            assert torch.equal(out.view.cpu(), torch.arange(n, dtype=torch.int32))


def test_sort_counts(cuda):
    """n = 0, 1, 2, 63, 64, 65; one workgroup's items +- 1; exactly two rounds per workgroup; three
    rounds with a ragged last one (sizes from msw_locality_launch)."""
    grid, per_wg, _ = loc.locality_launch(2 ** 26)
    sizes = [0, 1, 2, 63, 64, 65, per_wg - 1, per_wg, per_wg + 1, 2 * grid * per_wg, 2 * grid * per_wg + per_wg + 9]
    assert loc.locality_launch(sizes[-2]) == (grid, per_wg, 2)
    g3, _, it3 = loc.locality_launch(sizes[-1])
    assert it3 == 3 and g3 * 3 * per_wg > sizes[-1] + per_wg   # the last workgroup's run is ragged
    for n in sizes:
        st = check_sort(lc.sort_keys("random", n, seed=n + 1), cuda, label=f"n = {n}")
        if n:
            assert st.passes == 4 and st.n == n and st.scratch_bytes >= 12 * n
    check_sort(lc.sort_keys("three_values", sizes[-1]), cuda, label="long ties over three rounds")


def test_sort_segments(cuda):
    """Several segments, empty and one-item ones among them: every segment is sorted in place."""
    seg = [0, 0, 1, 300, 300, 301, 1500, 1500]
    keys = lc.sort_keys("random", 1500)
    keys[300:1500] = lc.sort_keys("three_values", 1200)
    st = check_sort(keys, cuda, seg, "7 segments")
    assert st.passes == 5 and st.num_segs == 7
    many = np.arange(0, 3001, 10)                # 300 segments: two passes over the segment index
    st = check_sort(lc.sort_keys("low_digit", 3000), cuda, many, "300 segments")
    assert st.passes == 6


def test_locality_refusals(cuda):
    lib = _lib.lib()
    k = torch.zeros(8, dtype=torch.int32, device=cuda)
    xy = torch.zeros(8, 2, dtype=torch.float64, device=cuda)
    out = Out((8,), cuda)
    dev, st = cuda.index or 0, stream_ptr()
    seg = lambda *v: np.array(v, np.int64).ctypes.data_as(_lib.c_int64_p)  # noqa: E731
    box = lambda *v: np.array(v, np.float64).ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    kp, xp = C.c_void_p(k.data_ptr()), C.c_void_p(xy.data_ptr())
    assert lib.msw_locality_sort(None, 8, seg(0, 8), 1, out.ptr, dev, st, None) == INVALID
    assert lib.msw_locality_sort(kp, 8, None, 1, out.ptr, dev, st, None) == INVALID
    assert lib.msw_locality_sort(kp, 8, seg(0, 8), 1, None, dev, st, None) == INVALID
    assert lib.msw_locality_sort(kp, -1, seg(0, 8), 1, out.ptr, dev, st, None) == INVALID
    for bad in ((1, 8), (0, 7), (0, 9, 8)):                         # does not tile [0, n)
        assert lib.msw_locality_sort(kp, 8, seg(*bad), len(bad) - 1, out.ptr, dev, st, None) == INVALID, bad
    assert lib.msw_locality_sort(C.c_void_p(k.data_ptr() + 2), 4, seg(0, 4), 1, out.ptr, dev, st, None) == INVALID
    assert lib.msw_locality_order(None, 8, seg(0, 8), 1, box(0, 0, 1), out.ptr, dev, st, None) == INVALID
    assert lib.msw_locality_order(xp, 8, seg(0, 8), 1, None, out.ptr, dev, st, None) == INVALID
    for side in (0.0, -1.0, float("inf"), float("nan"), 5e-324, 1e-304):   # the last two: 65536 / side overflows
        assert lib.msw_locality_order(xp, 8, seg(0, 8), 1, box(0, 0, side), out.ptr, dev, st, None) == INVALID
        assert lib.msw_hilbert_keys(xp, 8, 0.0, 0.0, side, out.ptr, st) == INVALID
    assert lib.msw_locality_order(C.c_void_p(xy.data_ptr() + 4), 4, seg(0, 4), 1, box(0, 0, 1), out.ptr, dev, st,
                                  None) == INVALID
    # n > 2^26: refused from the size alone, nothing of that size exists
    big = 2 ** 26 + 1
    assert lib.msw_locality_sort(kp, big, seg(0, big), 1, out.ptr, dev, st, None) == UNSUPPORTED
    assert lib.msw_locality_order(xp, big, seg(0, big), 1, box(0, 0, 1), out.ptr, dev, st, None) == UNSUPPORTED
    assert lib.msw_hilbert_keys(xp, big, 0.0, 0.0, 1.0, out.ptr, st) == UNSUPPORTED
    torch.cuda.synchronize()
    assert out.untouched()
    g, p, it = C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.msw_locality_launch(-1, C.byref(g), C.byref(p), C.byref(it)) == INVALID
    assert lib.msw_locality_launch(5, None, C.byref(p), C.byref(it)) == INVALID
    assert loc.locality_launch(0) == (0, 256, 0)


# ----------------------------------------------------------------------------- graph order
def test_row_order_gpu_equals_cpu(cuda):
    g, xy = lc.quadtree_graph(4, 3, seed=1)
    small = make_multiscale_mesh(n_coarse=4, num_scales=3, seed=1, T=2)
    irr, old = irregularize(small, 5)
    xi = xy[old].clone()
    xi[11] = float("nan")
    stats = {}
    got = loc.row_order(irr, xi.to(cuda), stats=stats)
    assert got.dtype == torch.int64 and got.device.type == "cpu" and torch.equal(got, loc.row_order(irr, xi))
    assert stats["passes"] == 5 and stats["num_segs"] == 3 and stats["sort_us"] > 0 and stats["keys_us"] > 0
    (ga, xa), (gb, xb) = lc.quadtree_graph(2, 3, seed=1), lc.quadtree_graph(3, 3, seed=2)
    batch = adapt_batch_training(collate([ga, gb]))
    bxy = torch.cat([xa, xb + 5000.0])
    assert torch.equal(loc.row_order(batch, bxy, device=cuda), loc.row_order(batch, bxy))
    assert torch.equal(loc.row_order(g, xy, device=cuda), loc.row_order(g, xy))


# ----------------------------------------------------------------------------- engine
T = 6
_XY = {}


def _small_xy():
    if "small" not in _XY:
        _XY["small"] = lc.quadtree_graph(**mesh_config("small"), seed=0)[1]
    return _XY["small"]


def _mesh(kind):
    """-> (graph on the CPU, row_xy) of one mesh kind."""
    small = wet_state(make_multiscale_mesh(**mesh_config("small"), T=T), seed=3)
    if kind == "quadtree":
        return small, _small_xy()
    if kind == "irregular":
        g, old = irregularize(small, 7, extra=("childless", "children16", "two_parents", "isolated", "ghost_first"))
        return g, _small_xy()[old]
    if kind == "batch":
        tiny = wet_state(make_multiscale_mesh(**mesh_config("tiny"), seed=11, T=T), seed=11)
        g, old = irregularize(small, 6)
        txy = lc.quadtree_graph(**mesh_config("tiny"), seed=11)[1]
        return adapt_batch_training(collate([g, tiny])), torch.cat([_small_xy()[old], txy])
    n0 = int(small.node_ptr[1])
    single = wet_state(make_single_scale_mesh(n_coarse=3, refinements=3, T=T), seed=3)
    if kind == "gnn_quadtree":
        return single, _small_xy()[:n0]
    assert kind == "gnn_irregular"
    g, old = irregularize(single, 7)
    return g, _small_xy()[:n0][old]


def _model(name):
    if name == "F16":
        return build_msgnn(4, 16, 2, state=weights("K2_F16"))
    if name == "F32":
        return build_msgnn(4, 32, 4, state=weights("K4_F32"))
    if name in ("F64", "F50"):
        return build_msgnn(4, int(name[1:]), 4)
    return build_gnn(state=weights("gnn_F32_seed42"))


def _orders(g, xy):
    ptr = np.unique(g.node_ptr.numpy().reshape(-1)) if "node_ptr" in g.keys() else np.array([0, g.num_nodes])
    rng = np.random.default_rng(17)
    return {"hilbert": loc.row_order(g, xy),
            "reversed": torch.from_numpy(np.concatenate([np.arange(b - 1, a - 1, -1) for a, b in zip(ptr[:-1], ptr[1:])])),
            "random": torch.from_numpy(np.concatenate([a + rng.permutation(b - a) for a, b in zip(ptr[:-1], ptr[1:])]))}


def _with_order(g, order):
    out = g.clone()
    out.row_order = order.to(g.x.device)
    return out


def _run(model, g, cuda):
    plan = EnginePlan(model, g, cuda)
    try:
        y = plan.forward(g.x).cpu()
        r = plan.rollout(g.x, g.BC, g.node_BC, g.type_BC, T).cpu()
        st = plan.stats()
        assert st["forward_calls"] >= 1 and st["rollout_steps"] >= T and st["kernels_per_step"] > 0
        return y, r, plan.row_layout()
    finally:
        plan.close()


CASES = [(m, k) for m in ("F16", "F32", "F64", "F50") for k in ("quadtree", "irregular", "batch")] + \
        [("GNN", "gnn_quadtree"), ("GNN", "gnn_irregular")]


@pytest.mark.parametrize("model,kind", CASES)
def test_ordered_plan_is_bit_identical(cuda, model, kind, monkeypatch):
    """One forward and a rollout of previous_t + 3 steps from a plan with a row order, against the plan
    without one: torch.equal, for the Hilbert, the reversed and a random order."""
    for k in ("MSW_GRID_CAP", "MSW_TILE_PACK"):
        monkeypatch.delenv(k, raising=False)
    g, xy = _mesh(kind)
    m = _model(model).to(cuda)
    gd = g.to(cuda)
    y0, r0, layout0 = _run(m, gd, cuda)
    assert r0.abs().max() > 0.01 and r0.shape[-1] == m.previous_t + 3
    for name, order in _orders(g, xy).items():
        y, r, layout = _run(m, _with_order(gd, order), cuda)
        assert torch.equal(y, y0), f"forward under the {name} order: {(y - y0).abs().max().item():.3e}"
        assert torch.equal(r, r0), f"rollout under the {name} order: {(r - r0).abs().max().item():.3e}"
        assert not np.array_equal(layout, layout0) and np.array_equal(np.sort(layout[layout >= 0]), np.arange(g.num_nodes))


def test_default_plan_vs_oracle(cuda):
    """What the ordered plans are compared with, against the oracle once."""
    g, _ = _mesh("quadtree")
    P, cfg = weights("K4_F32"), manifest()["weights_K4_F32_cfg"]
    y, r, _ = _run(_model("F32").to(cuda), g.to(cuda), cuda)
    assert rel_err(y, orc.forward(P, cfg, g)) <= REL_TOL
    assert per_step_rel(r, orc.rollout(P, cfg, g, T)) <= REL_TOL


def test_ordered_plan_under_a_grid_cap(cuda, monkeypatch):
    monkeypatch.setenv("MSW_GRID_CAP", "2")
    g, xy = _mesh("irregular")
    m = _model("F32").to(cuda)
    gd = g.to(cuda)
    y0, r0, _ = _run(m, gd, cuda)
    y, r, _ = _run(m, _with_order(gd, loc.row_order(g, xy)), cuda)
    assert torch.equal(y, y0) and torch.equal(r, r0)


def test_ordered_plan_in_the_reference_step_loop(cuda, monkeypatch):
    """The reference's rollout loop, one msw_forward per step."""
    monkeypatch.delenv("MSW_GRID_CAP", raising=False)
    g, xy = _mesh("irregular")
    m = _model("F32").to(cuda)
    dyn = 2 * m.previous_t
    outs = []
    for gd in (g.to(cuda), _with_order(g.to(cuda), loc.row_order(g, xy))):
        plan = EnginePlan(m, gd, cuda)
        x = gd.x.clone()
        preds = []
        for t in range(T):
            x[:, -dyn:] = apply_boundary_condition(x[:, -dyn:], gd.BC[:, :, t], gd.node_BC, type_BC=gd.type_BC)
            y = plan.forward(x)
            x = use_prediction(x, y, m.previous_t)
            preds.append(y.cpu())
        assert plan.stats()["forward_calls"] >= T
        plan.close()
        outs.append(torch.stack(preds, -1))
    assert outs[0].abs().max() > 0.01 and torch.equal(outs[0], outs[1])


def test_row_layout_shows_the_order(cuda, monkeypatch):
    g, xy = lc.quadtree_graph(8, 4, seed=0, T=T)
    gr, xyr, _ = lc.renumbered(g, xy, 9)
    order = loc.row_order(gr, xyr)
    m = build_msgnn(4, 32, 4, state=weights("K4_F32")).to(cuda)
    gd = _with_order(gr.to(cuda), order)
    monkeypatch.setenv("MSW_TILE_PACK", "0")
    plan = EnginePlan(m, gd, cuda)
    layout = plan.row_layout()
    plan.close()
    assert layout.dtype == np.int32 and len(layout) % 16 == 0 and (layout == -1).any()
    assert np.array_equal(layout[layout >= 0], order.numpy())          # exactly the order, padding apart
    monkeypatch.delenv("MSW_TILE_PACK")
    plan = EnginePlan(m, gd, cuda)
    layout = plan.row_layout()
    plan.close()
    rows = layout[layout >= 0].astype(np.int64)
    assert np.array_equal(np.sort(rows), np.arange(gr.num_nodes))       # a permutation
    generator, random, laid = loc.block_span(g), loc.block_span(gr), loc.block_span(gr, rows)
    print(f"block_span of the laid-out rows: {laid:.2f} (generator {generator:.2f}, random {random:.2f})")
    assert laid <= 2.0 * generator and laid <= random / 8.0


# ----------------------------------------------------------------------------- cache and refusals
def test_plan_cache_tells_orders_apart(cuda, monkeypatch):
    monkeypatch.delenv("MSW_GRID_CAP", raising=False)
    g, xy = _mesh("quadtree")
    m = _model("F32").to(cuda)
    gd = g.to(cuda)
    ordered = Graph(**gd.__dict__)                                      # the same tensors, plus an order
    ordered.row_order = loc.row_order(g, xy)
    p_plain, p_ord = plan_for(m, gd), plan_for(m, ordered)
    assert p_plain is not p_ord
    assert plan_for(m, ordered) is p_ord and plan_for(m, gd) is p_plain  # reused on a repeat call
    assert not np.array_equal(p_plain.row_layout(), p_ord.row_layout())
    y = p_ord.forward(gd.x)
    assert torch.equal(y, p_plain.forward(gd.x))
    a = int(g.node_ptr[0])
    ordered.row_order[[a, a + 1]] = ordered.row_order[[a + 1, a]]        # in place: still a valid order
    p_new = plan_for(m, ordered)
    assert p_new is not p_ord and p_ord._h is None                       # rebuilt, the stale plan closed
    assert torch.equal(p_new.forward(gd.x), y)
    assert plan_for(m, gd) is p_plain                                    # a graph without the attribute: as ever


def test_batch_of_ordered_graphs_plans(cuda, monkeypatch):
    """collate drops the members' row_order: a batch of ordered graphs plans like the batch of the
    same graphs without one, and runs through the model's own path (plan_for)."""
    from mswegnn.rollout import rollout_test
    monkeypatch.delenv("MSW_GRID_CAP", raising=False)
    small, xy = _mesh("quadtree")
    tiny = wet_state(make_multiscale_mesh(**mesh_config("tiny"), seed=11, T=T), seed=11)
    txy = lc.quadtree_graph(**mesh_config("tiny"), seed=11)[1]
    ordered = [_with_order(small, loc.row_order(small, xy)), _with_order(tiny, loc.row_order(tiny, txy))]
    m = _model("F32").to(cuda)
    m.engine = "hip"
    batch = collate(ordered)
    assert "row_order" not in batch.keys()
    r = rollout_test(m, batch.to(cuda)).cpu()
    r0 = rollout_test(m, collate([small, tiny]).to(cuda)).cpu()
    assert r0.abs().max() > 0.01 and torch.equal(r, r0)
    adapted = adapt_batch_training(batch).to(cuda)
    y0, q0, _ = _run(m, adapted, cuda)
    y, q, _ = _run(m, _with_order(adapted, loc.row_order(adapted, torch.cat([xy, txy]))), cuda)
    assert torch.equal(y, y0) and torch.equal(q, q0)                    # the order computed on the batch


def test_bad_orders_are_refused(cuda):
    g, xy = _mesh("quadtree")
    m = _model("F32").to(cuda)
    gd = g.to(cuda)
    good = loc.row_order(g, xy)
    n1 = int(g.node_ptr[1])

    def refused(order, word):
        with pytest.raises(_lib.EngineError) as e:
            EnginePlan(m, _with_order(gd, order), cuda)
        assert e.value.code == INVALID and word in str(e.value), str(e.value)

    refused(good[:-1], "row_order has shape")                            # the wrong length
    dup = good.clone()
    dup[5] = dup[4]
    refused(dup, "row_order[5]")
    for v in (-1, g.num_nodes):
        out = good.clone()
        out[3] = v
        refused(out, "row_order[3]")
    cross = good.clone()
    cross[[0, n1]] = cross[[n1, 0]]                                      # two entries swapped across a scale
    refused(cross, "row_order[0]")
    batch, bxy = _mesh("batch")
    bgood = loc.row_order(batch, bxy)
    b0 = int(batch.node_ptr[1, 0])                                       # first row of the second graph
    bcross = bgood.clone()
    bcross[[0, b0]] = bcross[[b0, 0]]                                    # ... and across a graph
    with pytest.raises(_lib.EngineError) as e:
        EnginePlan(m, _with_order(batch.to(cuda), bcross), cuda)
    assert e.value.code == INVALID and "row_order[0]" in str(e.value) and "outside its range" in str(e.value)
    with pytest.raises(ValueError, match="row order"):                   # partitioned plans take none
        EnginePlan(m, _with_order(gd, good), cuda, exchange=_lib.MswExchangeDesc(), rank=0)
    y0, r0, _ = _run(m, gd, cuda)                                        # the engine stays usable
    y, r, _ = _run(m, _with_order(gd, good), cuda)
    assert torch.equal(y, y0) and torch.equal(r, r0)
