"""The locality order without a GPU: the numpy restatement of the Hilbert keys checks itself (the
curve is a bijection whose consecutive cells are 4-neighbours; the quantisation at its edges), the
CPU path of mswegnn.locality.row_order equals it, block_span shows what the order is for, and the
host side of msw_plan_create_ordered (graph_build.h build_host_graph with a row order) runs under
AddressSanitizer + UndefinedBehaviorSanitizer in a stand-alone program (tests/asan/host_order_check.cpp).
"""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import locality_cases as lc
from conftest import ROOT
from mswegnn import locality as loc
from mswegnn.batch import collate
from mswegnn.mesh import irregularize, make_multiscale_mesh, make_single_scale_mesh, mesh_config, wet_state
from mswegnn.rollout import adapt_batch_training


# ----------------------------------------------------------------------------- the curve
@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
def test_curve_is_a_bijection_of_neighbouring_cells(order):
    n = 1 << order
    ii, jj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    d = lc.hilbert_index_ref(ii.ravel(), jj.ravel(), order)
    assert np.array_equal(np.sort(d), np.arange(n * n))
    along = np.argsort(d)
    step = np.abs(np.diff(ii.ravel()[along])) + np.abs(np.diff(jj.ravel()[along]))
    assert (step == 1).all()
    assert np.array_equal(loc._hilbert_index(ii.ravel(), jj.ravel(), order), d)  # the package's own restatement


def test_order_16_keys_nest():
    """The key of a cell of the 32 x 32 grid, at order 16, is the order-5 index in the top ten bits:
    coarser cells are contiguous key ranges, which is why one box serves every scale."""
    xy, box = lc.KEY_CASES["cell_centres_32"]
    keys = lc.hilbert_keys_ref(xy, box).astype(np.int64)
    cell = np.floor(xy * 32).astype(np.int64)
    assert np.array_equal(keys >> 22, lc.hilbert_index_ref(cell[:, 0], cell[:, 1], 5))


# ----------------------------------------------------------------------------- quantisation
def test_quantisation_edges():
    box = (10.0, -4.0, 8.0)                      # a cell is 2^-13 wide: every product below is exact
    h = 8.0 / 65536.0

    def cell(x, y=-4.0):
        """(ix, iy) recovered from the key of one point: along y = y0 the curve's first row."""
        k = int(lc.hilbert_keys_ref([[x, y]], box)[0])
        ii, jj = np.meshgrid(np.arange(65536, dtype=np.int64), np.zeros(1, np.int64), indexing="ij")
        return int(np.nonzero(lc.hilbert_index_ref(ii.ravel(), jj.ravel()) == k)[0][0])

    assert cell(10.0) == 0 and cell(10.0 + h) == 1                      # a point on a cell boundary belongs
    assert cell(np.nextafter(10.0 + h, -np.inf)) == 0                   # to the upper cell
    assert cell(10.0 + 7 * h) == 7 and cell(np.nextafter(10.0 + 7 * h, -np.inf)) == 6
    assert cell(18.0) == 65535 and cell(np.nextafter(18.0, -np.inf)) == 65535   # the far end clamps
    assert cell(1e300) == 65535 and cell(-1e300) == 0 and cell(9.0) == 0        # outside: clamped
    zero = (0.0, 0.0, 1.0)
    k = lc.hilbert_keys_ref([[-0.0, -0.0], [0.0, 0.0], [-0.0, 0.0]], zero)
    assert (k == 0).all()                                               # -0.0 is cell 0
    bad = [[np.nan, 0.5], [0.5, np.nan], [np.inf, 0.5], [0.5, -np.inf], [np.nan, np.inf]]
    assert (lc.hilbert_keys_ref(bad, zero) == lc.LAST_KEY).all()        # the last key
    assert lc.hilbert_keys_ref([[1.0, 0.0]], zero)[0] == lc.LAST_KEY    # ... which the curve's last cell shares
    with pytest.raises(ValueError):
        loc.hilbert_keys(np.zeros((1, 2)), (0.0, 0.0, 0.0))
    with pytest.raises(ValueError):
        loc.hilbert_keys(np.zeros((1, 2)), (0.0, 0.0, np.inf))
    with pytest.raises(ValueError):                                     # 65536 / side overflows: no cell
        loc.hilbert_keys(np.zeros((1, 2)), (0.0, 0.0, 5e-324))
    assert loc.bounding_square(np.array([[0.0, 0.0], [5e-324, 0.0]]))[2] == 1.0


@pytest.mark.parametrize("name", list(lc.KEY_CASES))
def test_cpu_keys_equal_the_restatement(name):
    xy, box = lc.KEY_CASES[name]
    got = loc.hilbert_keys(xy, box, device="cpu")
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), lc.hilbert_keys_ref(xy, box).astype(np.int64))


# ----------------------------------------------------------------------------- row_order, CPU path
def _want_order(graph, row_xy):
    """row_order from the restatement alone: per graph one bounding square, per range one argsort."""
    xy = row_xy.numpy()
    N = graph.num_nodes
    ptr = graph.node_ptr.numpy().reshape(-1, graph.node_ptr.shape[-1]) if "node_ptr" in graph.keys() \
        else np.array([[0, N]])
    out = np.full(N, -1, np.int64)
    for row in ptr:
        pts = xy[row[0]:row[-1]]
        pts = pts[np.isfinite(pts).all(1)]
        lo, hi = pts.min(0), pts.max(0)
        box = (lo[0], lo[1], max(hi[0] - lo[0], hi[1] - lo[1]))
        for a, b in zip(row[:-1], row[1:]):
            out[a:b] = a + lc.order_ref(lc.hilbert_keys_ref(xy[a:b], box))
    return out


def test_row_order_cpu_three_scales():
    g, xy = lc.quadtree_graph(4, 3, seed=1)
    g, xy, _ = lc.renumbered(g, xy, 5)
    xy = xy.clone()
    xy[7] = float("nan")                                  # a row without a position goes last in its range
    order = loc.row_order(g, xy)
    assert order.dtype == torch.int64 and order.device.type == "cpu"
    assert np.array_equal(order.numpy(), _want_order(g, xy))
    assert int(order[int(g.node_ptr[1]) - 1]) == 7
    for a, b in zip(g.node_ptr[:-1].tolist(), g.node_ptr[1:].tolist()):
        assert sorted(order[a:b].tolist()) == list(range(a, b))


def test_row_order_cpu_two_graph_batch():
    (ga, xa), (gb, xb) = lc.quadtree_graph(2, 3, seed=1), lc.quadtree_graph(3, 3, seed=2)
    xb = xb + 5000.0                                      # the second graph lies elsewhere: a box of its own
    batch = adapt_batch_training(collate([ga, gb]))
    assert batch.node_ptr.dim() == 2 and batch.node_ptr.shape == (2, 4)
    xy = torch.cat([xa, xb])
    order = loc.row_order(batch, xy)
    assert np.array_equal(order.numpy(), _want_order(batch, xy))
    # each member's part of the batch order is that member's own order, offset
    assert torch.equal(order[:ga.num_nodes], loc.row_order(ga, xa))
    assert torch.equal(order[ga.num_nodes:], loc.row_order(gb, xb) + ga.num_nodes)


def test_collate_drops_row_order():
    """collate does not carry a member's row_order (concatenated it would lack the offsets, and the
    plan would refuse it): a batch of ordered graphs has none, the engine sees no order in it, and
    the order of the batch is computed on the batch."""
    from mswegnn import engine
    from mswegnn.mesh import multiscale_geometry
    from mswegnn.meshgraph import graph_from_meshes
    mgs, plain = [], []
    for n_coarse, seed in ((2, 1), (3, 2)):
        geo = multiscale_geometry(n_coarse, 3, seed)
        dem = np.zeros(geo[0][1].shape[0])
        mgs.append(graph_from_meshes(geo, (0.0, 500.0), dem, T=2, locality=True))
        plain.append(graph_from_meshes(geo, (0.0, 500.0), dem, T=2).graph)
    members = [m.graph for m in mgs]
    assert all("row_order" in g.keys() for g in members)
    for batch in (collate(members), adapt_batch_training(collate(members)), collate(members).clone()):
        assert "row_order" not in batch.keys() and getattr(batch, "row_order", None) is None
        assert engine._row_order([], batch) is None
    batch, want = adapt_batch_training(collate(members)), adapt_batch_training(collate(plain))
    assert sorted(batch.keys()) == sorted(want.keys())                 # the batch of unordered graphs, exactly
    for k in want.keys():
        a, b = getattr(batch, k), getattr(want, k)
        assert torch.equal(a, b) if torch.is_tensor(a) else True, k
    assert all("row_order" in g.keys() for g in members)                # the members keep theirs
    order = loc.row_order(batch, torch.cat([m.row_xy for m in mgs]))
    for a, b in zip(batch.node_ptr[:, :-1].reshape(-1).tolist(), batch.node_ptr[:, 1:].reshape(-1).tolist()):
        assert sorted(order[a:b].tolist()) == list(range(a, b))
    n0 = members[0].num_nodes
    assert torch.equal(order[:n0], members[0].row_order) and torch.equal(order[n0:], members[1].row_order + n0)


def test_row_order_cpu_one_scale_gnn_graph():
    g, xy = lc.quadtree_graph(3, 4, seed=0)
    n0 = int(g.node_ptr[1])
    gs = make_single_scale_mesh(n_coarse=3, refinements=3, T=2)
    assert gs.num_nodes == n0 and "node_ptr" not in gs.keys()
    order = loc.row_order(gs, xy[:n0])
    assert np.array_equal(order.numpy(), _want_order(gs, xy[:n0]))
    assert sorted(order.tolist()) == list(range(n0))


def test_graph_from_meshes_locality_flag():
    from mswegnn.mesh import multiscale_geometry
    from mswegnn.meshgraph import graph_from_meshes
    geo = multiscale_geometry(3, 3, 0)
    dem = np.zeros(geo[0][1].shape[0])
    plain = graph_from_meshes(geo, (0.0, 500.0), dem, T=2)
    with_order = graph_from_meshes(geo, (0.0, 500.0), dem, T=2, locality=True)
    assert "row_order" not in plain.graph.keys()          # the default does not change
    g = with_order.graph
    assert torch.equal(g.row_order, loc.row_order(plain.graph, plain.row_xy))
    for k in plain.graph.keys():
        a, b = getattr(plain.graph, k), getattr(g, k)
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b, k
    # row_xy: centroids, the ghost at its BC face's, so the ghost follows that face in the order
    xy = plain.row_xy
    assert xy.dtype == torch.float64 and xy.shape == (g.num_nodes, 2)
    for s in range(3):
        a, ghost = int(g.node_ptr[s]), int(g.node_ptr[s + 1]) - 1
        assert torch.equal(xy[ghost], xy[a + plain.bc_face[s]])
        assert torch.equal(xy[a:ghost], plain.centroids[s])
    at = g.row_order.tolist().index(a + plain.bc_face[2])
    assert g.row_order[at + 1] == ghost
    assert torch.equal(g.clone().row_order, g.row_order) and torch.equal(g.to("cpu").row_order, g.row_order)


# ----------------------------------------------------------------------------- block_span
def test_block_span_of_the_hilbert_order():
    """Distinct 64-row source blocks per 16 consecutive destination rows, finest scale of the
    8,192-face mesh: the Hilbert order of a random numbering stays within 2 x the generator's
    (quadtree) numbering and at or below 1/8 of the random numbering itself."""
    g, xy = lc.quadtree_graph(8, 4, seed=0)
    gr, xyr, _ = lc.renumbered(g, xy, 9)
    generator, random = loc.block_span(g), loc.block_span(gr)
    ordered = loc.block_span(gr, loc.row_order(gr, xyr))
    print(f"block_span: generator {generator:.2f}, random {random:.2f}, random + Hilbert {ordered:.2f} "
          f"({ordered / generator:.2f} x, {ordered / random:.3f})")
    assert random > 8 * generator                         # the renumbering did destroy the locality
    assert ordered <= 2.0 * generator and ordered <= random / 8.0
    # the order is a property of the coordinates, not of the numbering
    assert abs(loc.block_span(g, loc.row_order(g, xy)) - ordered) < 0.05 * ordered


# ----------------------------------------------------------------------------- host plan, sanitizers
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("asan") / "host_order_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "mswe-gnn_amd", "csrc"), os.path.join(ROOT, "tests", "asan", "host_order_check.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_host_plan_with_a_row_order_under_asan_ubsan(harness, tmp_path):
    from test_host_sanitizer import _write_case
    path = tmp_path / "cases.bin"
    names = []

    def case(f, name, g, order):
        _write_case(f, name, g)
        f.write(np.asarray(order, np.int64).tobytes())
        names.append(name)

    def shuffled(g, seed):
        """A seeded random order: each range of node_ptr permuted in place."""
        rng = np.random.default_rng(seed)
        ptr = g.node_ptr.numpy().reshape(-1) if "node_ptr" in g.keys() else np.array([0, g.num_nodes])
        ptr = np.unique(ptr)
        return np.concatenate([a + rng.permutation(b - a) for a, b in zip(ptr[:-1], ptr[1:])])

    with open(path, "wb") as f:
        g, xy = lc.quadtree_graph(3, 4, seed=0)
        case(f, "quadtree_hilbert", g, loc.row_order(g, xy))
        case(f, "quadtree_random", g, shuffled(g, 1))
        small = wet_state(make_multiscale_mesh(**mesh_config("small"), T=2), seed=3)
        irr, old = irregularize(small, 5)
        case(f, "irregular_hilbert", irr, loc.row_order(irr, xy[old]))
        extras, old = irregularize(small, 7, extra=("childless", "children16", "two_parents", "isolated", "ghost_first"))
        case(f, "irregular_extras_reversed", extras,
             np.concatenate([np.arange(b - 1, a - 1, -1) for a, b in zip(extras.node_ptr[:-1].tolist(),
                                                                         extras.node_ptr[1:].tolist())]))
        batch = adapt_batch_training(collate([irregularize(small, 6)[0],
                                              make_multiscale_mesh(n_coarse=2, num_scales=4, seed=1, T=2)]))
        case(f, "batch_random", batch, shuffled(batch, 2))
        gs = make_single_scale_mesh(n_coarse=3, refinements=3, T=2)
        case(f, "gnn_single_scale_random", gs, shuffled(gs, 3))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([harness, str(path)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    recs = {x["case"]: x for x in (json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{"))}
    assert sorted(recs) == sorted(names)
    assert all(x["refusals"] >= 3 for x in recs.values())
    assert all(recs[n]["ranges_crossed"] == 1 for n in names if n != "gnn_single_scale_random")
