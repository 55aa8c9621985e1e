"""Irregular, renumbered meshes (mswegnn.mesh.irregularize) on the CPU: the generator's own
invariants, that its meshes really are irregular where the GPU tests need them to be, and the
oracle, the drop-in's torch path, collate and the decomposition on them.

make_multiscale_mesh is an exact 1->4 quadtree in hierarchical order; the reference's meshes
(database/graph_creation.py:422-436, 498-518, 922-927) have 2-6 children per coarse face,
fine faces without a parent, deleted faces and the mesh library's numbering.  The helpers
here (`irregular`, `back`, GPU_SEEDS) are shared with tests/test_gpu_irregular.py.
"""
import numpy as np
import pytest
import torch

from conftest import REL_TOL, build_gnn, build_msgnn, manifest, per_step_rel, rel_err, state_dict_of, weights
import msgnn_torch as orc
from mswegnn.mesh import (irregularize, make_multiscale_mesh, make_single_scale_mesh, mesh_config,
                          wet_state)

GPU_SEEDS = (0, 1, 2, 3)  # the irregularize seeds tests/test_gpu_irregular.py draws its meshes from
EXTRAS = ("childless", "children16", "children17", "two_parents", "isolated", "ghost_first")


@pytest.fixture(autouse=True)
def _threads():
    torch.set_num_threads(min(8, torch.get_num_threads()))


def irregular(name="small", seed=0, wet=None, all_wet=False, T=6, num_scales=None, **kw):
    """(graph, old_of_new, quadtree graph) of a named mesh_config after irregularize(seed);
    wet: wet_state seed (None = dry start) or all_wet."""
    cfg = dict(mesh_config(name))
    if num_scales is not None:
        cfg["num_scales"] = num_scales
    g0 = make_multiscale_mesh(**cfg, T=T)
    if wet is not None or all_wet:
        g0 = wet_state(g0, seed=wet or 0, all_wet=all_wet)
    g, old = irregularize(g0, seed, **kw)
    return g, old, g0


def back(r, old_of_new, n_old):
    """Rows of `r` (output numbering) scattered to the input numbering; deleted rows stay 0."""
    full = torch.zeros((n_old,) + tuple(r.shape[1:]), dtype=r.dtype)
    full[torch.from_numpy(np.asarray(old_of_new))] = r
    return full


def _levels(g):
    npt, ipt, ie = g.node_ptr.numpy(), g.intra_edge_ptr.numpy(), g.intra_mesh_edge_index.numpy()
    return npt, [ie[:, ipt[l]:ipt[l + 1]] for l in range(len(npt) - 2)]


def _edge_set(g, old):
    """The mesh in input ids, order-free: sorted dual edges with their attribute, sorted pairs."""
    ei = old[g.edge_index.numpy()]
    ea = g.edge_attr.numpy()[:, 0]
    k = np.lexsort((ei[1], ei[0]))
    pairs = old[g.intra_mesh_edge_index.numpy()] if "intra_mesh_edge_index" in g else np.zeros((2, 0), np.int64)
    return ei[:, k], ea[k], pairs[:, np.lexsort((pairs[1], pairs[0]))]


# ------------------------------------------------------------------ generator invariants
@pytest.mark.parametrize("S", [2, 3, 4])
@pytest.mark.parametrize("seed", range(8))
def test_generator_invariants(seed, S):
    g0 = wet_state(make_multiscale_mesh(n_coarse=3, num_scales=S, seed=seed, T=3), seed=seed)
    N0 = g0.num_nodes
    ref = None
    for permute in (False, True):
        for order in ("kept", "canonical"):
            g, old = irregularize(g0, seed, permute=permute, order=order)
            N, E = g.num_nodes, g.edge_index.shape[1]
            npt, ept = g.node_ptr.numpy(), g.edge_ptr.numpy()
            ei = g.edge_index.numpy()
            # pointers: monotone, spanning, one row fewer per deleted face, only on the finest scale
            assert npt[0] == 0 and npt[-1] == N and np.all(np.diff(npt) > 0) and len(npt) == S + 1
            assert ept[0] == 0 and ept[-1] == E and np.all(np.diff(ept) > 0)
            assert np.array_equal(np.diff(npt)[1:], np.diff(g0.node_ptr.numpy())[1:])
            assert N0 - N == round(0.03 * (int(g0.node_ptr[1]) - 2))
            assert g.edge_attr.shape[0] == E and g.y.shape[0] == N and g.area.shape[0] == N
            # old_of_new injective, scale-preserving
            assert len(old) == N and len(np.unique(old)) == N
            onp = g0.node_ptr.numpy()
            for s in range(S):
                assert np.all((old[npt[s]:npt[s + 1]] >= onp[s]) & (old[npt[s]:npt[s + 1]] < onp[s + 1]))
                e = ei[:, ept[s]:ept[s + 1]]
                assert np.all((e >= npt[s]) & (e < npt[s + 1])), "edge leaves its scale"
                # ghosts last in their scale, one directed ghost -> BC-face edge, last of the scale
                assert old[npt[s + 1] - 1] == onp[s + 1] - 1
                assert e[0, -1] == npt[s + 1] - 1 and (e == npt[s + 1] - 1).sum() == 1
                if order == "canonical":
                    key = e[0, :-1] * N + e[1, :-1]
                    assert np.all(np.diff(key) > 0)
            # every undirected dual edge still has both directions
            both = set(map(tuple, ei.T.tolist()))
            assert all((c, r) in both for r, c in both if r not in npt[1:] - 1)
            # intra pairs: (coarse, fine) of the right level, the ghost pair kept
            ipt = g.intra_edge_ptr.numpy()
            assert ipt[0] == 0 and ipt[-1] == g.intra_mesh_edge_index.shape[1] and len(ipt) == S
            for l, p in enumerate(_levels(g)[1]):
                assert np.all((p[0] >= npt[l + 1]) & (p[0] < npt[l + 2]) & (p[1] >= npt[l]) & (p[1] < npt[l + 1]))
                assert ((p[0] == npt[l + 2] - 1) & (p[1] == npt[l + 1] - 1)).sum() == 1
                assert (p[0] == npt[l + 2] - 1).sum() == 1, "a face was moved under the ghost"
                assert len(np.unique(p[1])) == p.shape[1], "a fine face has two parents"
                if order == "canonical":
                    assert np.all(np.diff(p[0] * N + p[1]) > 0)
            # carried fields follow the rows; BC and friends untouched
            idx = torch.from_numpy(old)
            assert torch.equal(g.x, g0.x[idx]) and torch.equal(g.area, g0.area[idx])
            assert old[int(g.node_BC[0])] == int(g0.node_BC[0]) and g.node_BC.dtype == g0.node_BC.dtype
            assert torch.equal(g.BC, g0.BC) and torch.equal(g.edge_BC_length, g0.edge_BC_length)
            for k in ("edge_index", "edge_ptr", "node_ptr", "intra_mesh_edge_index", "intra_edge_ptr", "x", "edge_attr"):
                assert getattr(g, k).dtype == getattr(g0, k).dtype, k
            # the same edited mesh under every labelling
            es = _edge_set(g, old)
            if ref is None:
                ref = (np.sort(old), es)
            else:
                assert np.array_equal(ref[0], np.sort(old))
                assert all(np.array_equal(a, b) for a, b in zip(ref[1], es))
    # deterministic per seed; other seeds differ
    a, oa = irregularize(g0, seed)
    b, ob = irregularize(g0, seed)
    assert np.array_equal(oa, ob) and torch.equal(a.edge_index, b.edge_index)
    assert not np.array_equal(oa, irregularize(g0, seed + 100)[1])


def test_identity_at_rate_zero():
    for g0 in (wet_state(make_multiscale_mesh(**mesh_config("small"), T=3), seed=1),
               wet_state(make_single_scale_mesh(n_coarse=3, refinements=2, T=3), seed=1)):
        for order in ("kept", "canonical"):  # the generator's own order is the canonical one
            g, old = irregularize(g0, 7, move=0, orphan=0, delete=0, permute=False, order=order)
            assert np.array_equal(old, np.arange(g0.num_nodes))
            assert g.keys() == g0.keys()
            for k in g0.keys():
                v = getattr(g0, k)
                assert torch.equal(getattr(g, k), v) if isinstance(v, torch.Tensor) else getattr(g, k) == v, k


def test_single_scale_mesh_with_deleted_faces():
    g0 = wet_state(make_single_scale_mesh(n_coarse=3, refinements=3, T=4), seed=2)
    g, old = irregularize(g0, 3)
    assert "node_ptr" not in g and g.num_nodes == g0.num_nodes - round(0.03 * (g0.num_nodes - 2))
    assert old[int(g.node_BC[0])] == int(g0.node_BC[0]) and int(g.node_BC[0]) == g.num_nodes - 1
    deg = np.bincount(g.edge_index[1].numpy(), minlength=g.num_nodes)
    assert (deg == 1).any() and (deg == 2).any() and deg.max() == 3


@pytest.mark.parametrize("seed", GPU_SEEDS)
def test_mesh_is_really_irregular(seed):
    """Conditions the GPU tests rely on, at the default rates on `small`: every level with at
    least 16 coarse faces has a coarse face with more than 4 children (beyond the inline pooling
    record), one with fewer than 4 and an orphan; the finest scale has rows of in-degree 1 and 2."""
    g, old, _ = irregular("small", seed, wet=seed)
    npt, levels = _levels(g)
    checked = 0
    for l, p in enumerate(levels):
        nc = npt[l + 2] - npt[l + 1]
        if nc < 16:
            continue
        checked += 1
        cnt = np.bincount(p[0] - npt[l + 1], minlength=nc)
        assert cnt.max() > 4 and cnt.min() < 4, (l, cnt.min(), cnt.max())
        assert (npt[l + 1] - npt[l]) - len(np.unique(p[1])) >= 1, f"no orphan on level {l}"
    assert checked == 3
    deg = np.bincount(g.edge_index[1].numpy(), minlength=g.num_nodes)[:npt[1]]
    assert (deg == 1).any() and (deg == 2).any()


def test_extras_build_the_named_structures():
    g0 = wet_state(make_multiscale_mesh(**mesh_config("small"), T=3), seed=2)
    base, ob = irregularize(g0, 2, permute=False)
    onp = g0.node_ptr.numpy()

    def children(g, old, level):
        npt, levels = _levels(g)
        p = old[levels[level]]
        return np.bincount(p[0] - onp[level + 1], minlength=onp[level + 2] - onp[level + 1]), p
    for permute in (False, True):
        g, old = irregularize(g0, 2, permute=permute, extra=("childless",))
        assert children(g, old, 0)[0][1] == 0 and children(base, ob, 0)[0][1] > 0
        for n in (16, 17):
            g, old = irregularize(g0, 2, permute=permute, extra=(f"children{n}",))
            cnt = children(g, old, 0)[0]
            assert cnt[0] == n and cnt[1:].max() <= 16
        g, old = irregularize(g0, 2, permute=permute, extra=("two_parents",))
        p = children(g, old, 1)[1]
        f, c = np.unique(p[1], return_counts=True)
        assert (c == 2).sum() == 1 and c.max() == 2 and len(np.unique(p[0][p[1] == f[c == 2][0]])) == 2
        assert all(len(np.unique(q[1])) == q.shape[1] for q in (children(g, old, 0)[1], children(g, old, 2)[1]))
        g, old = irregularize(g0, 2, permute=permute, extra=("isolated",))
        n0 = int(g.node_ptr[1])
        deg = np.bincount(g.edge_index[1].numpy(), minlength=g.num_nodes)[:n0]
        out = np.bincount(g.edge_index[0].numpy(), minlength=g.num_nodes)[:n0]
        bdeg = np.bincount(base.edge_index[1].numpy(), minlength=base.num_nodes)[:n0]
        assert (deg == 0).sum() == (bdeg == 0).sum() + 1 and ((deg == 0) & (out == 0)).sum() >= 1
        assert g.edge_index.shape[1] == base.edge_index.shape[1] - 6 and g.num_nodes == base.num_nodes
        g, old = irregularize(g0, 2, permute=permute, extra=("ghost_first",))
        assert int(g.node_BC[0]) == 0 and old[0] == onp[1] - 1
        e0 = g.edge_index[:, :int(g.edge_ptr[1])]
        assert int(e0[0, -1]) == 0 and int((e0 == 0).sum()) == 1
    g, old = irregularize(g0, 2, extra=EXTRAS[:2] + EXTRAS[3:])  # they compose
    cnt = children(g, old, 0)[0]
    assert cnt[0] == 16 and cnt[1] == 0
    with pytest.raises(ValueError):
        irregularize(g0, 2, extra=("children16", "children17"))
    with pytest.raises(ValueError):
        irregularize(g0, 2, extra=("nonsense",))


# ------------------------------------------------------------------ oracle, drop-in, collate
def test_oracle_is_exact_under_relabelling_and_close_under_reordering():
    """order="kept" changes ids only: every per-destination and per-parent sum adds the same
    terms in the same order, so the oracle's rollout mapped back is bit-identical.  One thing in
    the reference's arithmetic does depend on where a row sits: the residual's [N, 3] @ [3]
    product (models/models.py:50-77) is a BLAS matrix-vector call whose last N mod 16 rows are
    rounded by a remainder loop (seen here as one 1.5e-8 difference on a coarse face that one
    labelling puts there).  The delete share is therefore set so that N = 16 k + 1: the
    remainder is the coarsest ghost alone, the last row under every labelling.
    order="canonical" re-sorts each destination's in-edges, so sums reorder: REL_TOL."""
    P, cfg, T = weights("K4_F32"), manifest()["weights_K4_F32_cfg"], 6
    for seed, wet in ((0, 0), (3, None), (5, 5)):
        deleted = 29  # small: 1,534 rows - 29 = 16 * 94 + 1
        kw = dict(wet=wet, T=T, delete=deleted / 1151)
        ga, oa, g0 = irregular("small", seed, permute=False, order="kept", **kw)
        assert ga.num_nodes % 16 == 1
        gb, ob, _ = irregular("small", seed, permute=True, order="kept", **kw)
        gc, oc, _ = irregular("small", seed, permute=True, order="canonical", **kw)
        assert not np.array_equal(oa, ob)
        ra, rb, rc = (back(orc.rollout(P, cfg, g, T), o, g0.num_nodes) for g, o in ((ga, oa), (gb, ob), (gc, oc)))
        assert ra.abs().max() > 0.1
        assert torch.equal(ra, rb), (seed, (ra - rb).abs().max().item())
        e = per_step_rel(rc, ra)
        print(f"seed {seed}: canonical vs kept order, per-step rel {e:.2e}")
        assert e <= REL_TOL
    # the forward alone (no fed-back state) is exact at the default rates as well
    ga, oa, g0 = irregular("small", 5, wet=5, T=T, permute=False, order="kept")
    gb, ob, _ = irregular("small", 5, wet=5, T=T, permute=True, order="kept")
    assert torch.equal(back(orc.forward(P, cfg, ga), oa, g0.num_nodes), back(orc.forward(P, cfg, gb), ob, g0.num_nodes))
    # ... and where the default-rate rollout (N = 1,499 = 16 * 93 + 11) does depend on the
    # labelling, it is by that remainder: at the first step that differs, every row that differs
    # sits in the last N mod 16 rows under exactly one of the two labellings
    N = ga.num_nodes
    ra, rb = (back(orc.rollout(P, cfg, g, T), o, g0.num_nodes) for g, o in ((ga, oa), (gb, ob)))
    pos_a, pos_b = (np.full(g0.num_nodes, -1) for _ in range(2))
    pos_a[oa], pos_b[ob] = np.arange(N), np.arange(N)
    for t in range(T):
        rows = torch.nonzero((ra[..., t] != rb[..., t]).any(1)).flatten().numpy()
        if len(rows):
            print(f"default rates: step {t}, rows {rows.tolist()} differ by {(ra[..., t] - rb[..., t]).abs().max():.1e}")
            assert np.all((pos_a[rows] >= N // 16 * 16) != (pos_b[rows] >= N // 16 * 16)), (pos_a[rows], pos_b[rows])
            break


def test_reference_residual_product_rounds_its_remainder_rows_differently():
    """The cause named above, on the product itself (oracle residual = models/models.py:50-77,
    learned_residuals=True): permuting the rows of x permutes the result, bit for bit, except
    for rows that sit in the last N mod 16 rows in one order and not in the other.  (A BLAS
    without that remainder loop passes as well: no row differs.)"""
    P, cfg = weights("K4_F32"), manifest()["weights_K4_F32_cfg"]
    for N in (1499, 1505, 1488):
        tail = N // 16 * 16
        for trial in range(10):
            gen = torch.Generator().manual_seed(trial)
            x = torch.rand(N, 8, generator=gen)
            perm = torch.randperm(N, generator=gen)
            a, b = orc.residual(P, cfg, x)[perm], orc.residual(P, cfg, x[perm])
            k = torch.nonzero((a != b).any(1)).flatten()
            assert bool(((perm[k] >= tail) != (k >= tail)).all()), (N, trial, k.tolist())
            assert (a - b).abs().max() <= 2e-7 * a.abs().max()


def test_drop_in_torch_path_matches_oracle_bitwise():
    g, _, _ = irregular("small", 1, wet=1)
    m = build_msgnn(4, 32, 4, state=weights("K4_F32"))
    m.engine = "torch"
    with torch.no_grad():
        assert torch.equal(m(g), orc.forward(weights("K4_F32"), manifest()["weights_K4_F32_cfg"], g))
    gs, _ = irregularize(wet_state(make_single_scale_mesh(n_coarse=3, refinements=3, T=4), seed=2), 3)
    mg = build_gnn(state=weights("gnn_F32_seed42"))
    mg.engine = "torch"
    with torch.no_grad():
        assert torch.equal(mg(gs), orc.forward(weights("gnn_F32_seed42"), manifest()["weights_gnn_F32_seed42_cfg"], gs))
    for extra in ("two_parents", "childless", "isolated", "ghost_first"):
        g, _, _ = irregular("tiny", 2, wet=2, extra=(extra,))
        with torch.no_grad():
            assert torch.equal(m(g), orc.forward(state_dict_of(m), manifest()["weights_K4_F32_cfg"], g)), extra


def test_collate_irregular_and_regular_matches_individual_oracle():
    from mswegnn.batch import collate
    from mswegnn.rollout import adapt_batch_training
    ga, _, _ = irregular("small", 2, wet=2, T=3)
    gb = make_multiscale_mesh(n_coarse=2, num_scales=4, seed=2, T=3)
    bt = adapt_batch_training(collate([ga, gb]))
    assert tuple(bt.node_ptr.shape) == (2, 5)
    P, cfg = weights("K4_F32"), manifest()["weights_K4_F32_cfg"]
    r = orc.rollout(P, cfg, bt)
    ra, rb = orc.rollout(P, cfg, ga), orc.rollout(P, cfg, gb)
    na = ga.num_nodes
    # batched CPU matmuls block rows differently: equal to float rounding, not bit for bit
    assert rel_err(r[:na], ra) <= 1e-5 and rel_err(r[na:], rb) <= 1e-5


# ------------------------------------------------------------------ decomposition
@pytest.mark.parametrize("parts", [2, 3, 5])
def test_partition_of_an_irregular_mesh(parts):
    """tests/test_host_cpu.py::test_partition_invariants_and_halo_exchange on a mesh with moved
    pairs, orphans (no parent to follow), deleted faces and permuted ids."""
    from mswegnn import partition as P
    from test_host_cpu import _hops_global, _hops_part
    g, _, _ = irregular("small", 1, wet=1, T=4)
    owner, lps, xp = P.decompose(g, parts)
    npt = g.node_ptr.numpy()
    N = int(npt[-1])
    ii = g.intra_mesh_edge_index.numpy()
    assert owner.min() == 0 and owner.max() == parts - 1
    assert np.array_equal(owner[ii[1]], owner[ii[0]])  # pooling / unpooling never cross parts
    counts = np.bincount(owner[npt[0]:npt[1]], minlength=parts)
    # balance: the coarsest scale is cut at the midpoints of its faces' cumulative weight (finest
    # descendants), so a part's rooted weight is within one coarsest face's weight of the mean
    # -- the heaviest one here, where the quadtree's are all equal -- and the finest faces with
    # an orphan among their ancestors (not weighed by the cut) come on top
    root = np.arange(N)
    parent = np.full(N, -1, np.int64)
    parent[ii[1]] = ii[0]
    for s in range(len(npt) - 2, -1, -1):
        rows = np.arange(npt[s], npt[s + 1])
        root[rows] = np.where(parent[rows] >= 0, root[np.maximum(parent[rows], 0)], rows)
    fine_root = root[npt[0]:npt[1]]
    rooted = fine_root >= npt[-2]
    grain = np.bincount(fine_root[rooted] - npt[-2]).max()
    assert grain > -(-(npt[1] - npt[0]) // (npt[-1] - npt[-2]))  # uneven, unlike the quadtree
    assert counts.max() - counts.min() <= 2 * grain + (~rooted).sum(), (counts, grain, (~rooted).sum())
    # an orphan lives with a dual neighbour (or, isolated, anywhere), not all on rank 0
    has_parent = np.zeros(N, bool)
    has_parent[ii[1]] = True
    ei = g.edge_index.numpy()
    for v in np.nonzero(~has_parent[:npt[-2]])[0]:
        nb = ei[0][ei[1] == v]
        assert len(nb) == 0 or owner[v] in owner[nb], v
    seen = np.zeros(N, np.int64)
    for lp in lps:
        seen[lp.nodes[lp.owned]] += 1
        lnp = lp.graph.node_ptr.numpy()
        for s in range(len(npt) - 1):
            assert np.all(lp.scale_of[lnp[s]:lnp[s + 1]] == s)
            assert np.all((lp.nodes[lnp[s]:lnp[s + 1]] >= npt[s]) & (lp.nodes[lnp[s]:lnp[s + 1]] < npt[s + 1]))
        le = lp.nodes[lp.graph.edge_index.numpy()]
        want = np.isin(ei[1], lp.nodes[lp.owned])
        assert np.array_equal(le, ei[:, want])
        # every intra pair of an owned fine face is local, in reference order
        li = lp.nodes[lp.graph.intra_mesh_edge_index.numpy()]
        assert np.array_equal(li, ii[:, np.isin(ii[1], lp.nodes[lp.owned])])
    assert np.all(seen == 1)
    for p in range(parts):
        for s, peers in xp[p].items():
            for q, (recv, send) in peers.items():
                back_recv, back_send = xp[q][s][p]
                assert np.array_equal(lps[p].nodes[recv], lps[q].nodes[back_send])
                assert np.array_equal(lps[p].nodes[send], lps[q].nodes[back_recv])
                assert np.all(owner[lps[p].nodes[recv]] == q) and np.all(lps[q].owned[back_send])
    rng = np.random.default_rng(0)
    x = rng.standard_normal((N, 3))
    ref = _hops_global(g, x.copy(), 4)
    xls = [x[lp.nodes].copy() for lp in lps]
    for h in range(4):
        for p, lp in enumerate(lps):
            for s, peers in xp[p].items():
                for q, (recv, _) in peers.items():
                    if len(recv):
                        xls[p][recv] = xls[q][xp[q][s][p][1]]
        for p, lp in enumerate(lps):
            xls[p] = _hops_part(lp, xls[p], lambda xl: None, 1)
    out = P.assemble(lps, [torch.from_numpy(a) for a in xls], N).numpy()
    assert np.isfinite(out).all()
    np.testing.assert_allclose(out, ref, rtol=1e-12, atol=1e-12)
