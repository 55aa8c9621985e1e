"""The yardstick of the mesh graphs (mswegnn.meshgraph, msw_locator_* / msw_mesh_dual_*): brute-force
numpy restatements of include/mswegnn.h "Mesh graphs" -- ``locate_ref`` tries EVERY face at every
point with raster_cases' ``contains`` (no buckets, no bounding boxes), ``dual_ref`` is a dict of
edges, ``intra_ref`` the containment rule, ``graph_ref`` the assembly of mswegnn.mesh's layout --
and the named cases.  Indices are decided by fp64 predicates or vertex lists and the float64 arrays
are stated sequences of IEEE operations, so every comparison is bit for bit.

Each wrong ``variant`` must change an asserted array on a named case
(tests/test_meshgraph.py::test_sensitivity).
"""
import numpy as np

import raster_cases as rc
from mswegnn.mesh import _coarse_triangulation, _smooth_dem, _standardize, hydrograph_bc, multiscale_geometry

CANARY_I = rc.CANARY_I

LOCATE_VARIANTS = ("strict", "highest")
DUAL_VARIANTS = ("cols_unsorted", "slots_rotated")
INTRA_VARIANTS = ("fine_major",)
GRAPH_VARIANTS = ("no_ghost_edge", "ghost_edge_first", "ghost_row_first", "bc_not_overridden", "ghost_pooled")


# ----------------------------------------------------------------------------- restatements
def locate_ref(node_xy, face_nodes, face_row, pts, variant=None):
    """rows [n] int32: every face at every point; the last writer wins."""
    xy = np.asarray(node_xy, np.float64)
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    nf = len(face_nodes)
    rows = np.arange(nf, dtype=np.int32) if face_row is None else np.asarray(face_row, np.int32)
    out = np.full(pts.shape[0], -1, np.int32)
    with np.errstate(invalid="ignore"):
        for f in (range(nf) if variant == "highest" else range(nf - 1, -1, -1)):
            out[rc.contains(xy, face_nodes[f], pts[:, 0], pts[:, 1], variant)] = rows[f]
    return out


def dual_ref(node_xy, face_nodes, variant=None):
    """-> dict of centroid, area, adjacent, edge_index, edge_length, boundary from a dict of edges."""
    xy = np.asarray(node_xy, np.float64)
    nf = len(face_nodes)
    e2f = {}
    for f, (a, b, c) in enumerate(np.asarray(face_nodes).tolist()):
        for u, v in ((a, b), (b, c), (c, a)):
            e2f.setdefault((min(u, v), max(u, v)), []).append(f)
    centroid, area = np.zeros((nf, 2)), np.zeros(nf)
    adjacent = np.full((nf, 3), -1, np.int32)
    pairs, boundary = [], []
    for f, (a, b, c) in enumerate(np.asarray(face_nodes).tolist()):
        pa, pb, pc = xy[a], xy[b], xy[c]
        centroid[f] = ((pa + pb) + pc) / 3.0
        area[f] = 0.5 * abs((pb[0] - pa[0]) * (pc[1] - pa[1]) - (pc[0] - pa[0]) * (pb[1] - pa[1]))
        slots = ((b, c), (c, a), (a, b)) if variant == "slots_rotated" else ((a, b), (b, c), (c, a))
        for k, (u, v) in enumerate(slots):
            faces = e2f[(min(u, v), max(u, v))]
            assert len(faces) <= 2
            if len(faces) == 2:
                adjacent[f, k] = faces[0] if faces[1] == f else faces[1]
                pairs.append((f, int(adjacent[f, k])))
            else:
                boundary.append((f, k))
    if variant != "cols_unsorted":
        pairs = sorted(pairs)
    ei = np.asarray(pairs, np.int64).reshape(-1, 2).T
    d = centroid[ei[1]] - centroid[ei[0]]
    return dict(centroid=centroid, area=area, adjacent=adjacent, edge_index=ei,
                edge_length=np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]),
                boundary=np.asarray(boundary, np.int32).reshape(-1, 2))


def intra_ref(fine_centroid, coarse_xy, coarse_faces, variant=None):
    """(coarse, fine) pairs int64 [2, n]: coarse-major, fine ascending."""
    parent = locate_ref(coarse_xy, coarse_faces, None, fine_centroid)
    pairs = [(int(p), f) for f, p in enumerate(parent) if p >= 0]
    pairs = sorted(pairs, key=(lambda t: (t[1], t[0])) if variant == "fine_major" else None)
    return np.asarray(pairs, np.int64).reshape(-1, 2).T


def graph_ref(scales, bc_xy, dem, previous_t=3, T=48, BC=None, variant=None):
    """The arrays of ``graph_from_meshes(...).graph`` as a dict of numpy arrays, plus ``bc_face``,
    ``orphans`` and ``childless`` per scale, from the restatements above."""
    S = len(scales)
    point = np.asarray(bc_xy, np.float64)
    sc = []
    for xy, fn in scales:
        xy, fn = np.asarray(xy, np.float64), np.asarray(fn)
        d = dual_ref(xy, fn)
        best = None
        for f, k in d["boundary"].tolist():           # nearest midpoint, ties to the lowest (face, slot)
            u, v = fn[f, k], fn[f, (k + 1) % 3]
            mid = 0.5 * (xy[u] + xy[v])
            mx, my = mid[0] - point[0], mid[1] - point[1]
            dist2 = mx * mx + my * my
            if best is None or dist2 < best[0]:
                best = (dist2, f, u, v, mid)
        _, f, u, v, mid = best
        if variant != "bc_not_overridden":
            point = mid
        ex, ey = xy[v, 0] - xy[u, 0], xy[v, 1] - xy[u, 1]
        elen = np.sqrt(ex * ex + ey * ey)
        cross = ex * (d["centroid"][f, 1] - xy[u, 1]) - ey * (d["centroid"][f, 0] - xy[u, 0])
        nf = len(fn)
        ghost = np.array([[nf], [f]], np.int64)
        if variant == "no_ghost_edge":
            ei, dist = d["edge_index"], d["edge_length"]
        elif variant == "ghost_edge_first":
            ei, dist = np.concatenate([ghost, d["edge_index"]], 1), np.append(2.0 * (abs(cross) / elen), d["edge_length"])
        else:
            ei, dist = np.concatenate([d["edge_index"], ghost], 1), np.append(d["edge_length"], 2.0 * (abs(cross) / elen))
        sc.append(dict(xy=xy, fn=fn, nf=nf, c=d["centroid"], area=np.append(d["area"], d["area"][f]), ei=ei, dist=dist,
                       bc_face=f, bc_edge_len=elen))
    dems = [np.asarray(v, np.float64) for v in dem] if isinstance(dem, (list, tuple)) else [np.asarray(dem, np.float64)]
    parents, orphans, childless = [], [0] * S, [0] * S
    for s in range(S - 1):
        fine, coarse = sc[s], sc[s + 1]
        parent = locate_ref(coarse["xy"], coarse["fn"], None, fine["c"]).astype(np.int64)
        parents.append(parent)
        orphans[s] = int((parent < 0).sum())
        total, cnt = np.zeros(coarse["nf"]), np.zeros(coarse["nf"], np.int64)
        if len(dems) == s + 1:
            for f in range(fine["nf"]):               # ascending child order
                if parent[f] >= 0:
                    total[parent[f]] += dems[s][f]
                    cnt[parent[f]] += 1
            if variant == "ghost_pooled" and parent[fine["bc_face"]] >= 0:
                total[parent[fine["bc_face"]]] += dems[s][fine["bc_face"]]
                cnt[parent[fine["bc_face"]]] += 1
            d = total / np.maximum(cnt, 1)
            for f in np.nonzero(cnt == 0)[0]:
                under = locate_ref(fine["xy"], fine["fn"], None, coarse["c"][f][None])[0]
                assert under >= 0
                d[f] = dems[s][under]
            dems.append(d)
        else:
            cnt = np.bincount(parent[parent >= 0], minlength=coarse["nf"])
        childless[s + 1] = int((cnt == 0).sum())
    dem_min = min(d.min() for d in dems)
    face_ptr = np.cumsum([0] + [d["nf"] + 1 for d in sc])
    N = int(face_ptr[-1])
    x = np.zeros((N, 2 + 2 * previous_t), np.float32)
    area_raw = np.zeros(N)
    node_bc = face_ptr[0] + sc[0]["nf"]
    eis, attrs, intra = [], [], []
    for s, d in enumerate(sc):
        rows = np.arange(face_ptr[s], face_ptr[s + 1])
        dm = np.append(dems[s] - dem_min, (dems[s] - dem_min)[d["bc_face"]])
        ar, raw, ei = _standardize(d["area"]), d["area"], d["ei"].copy()
        if variant == "ghost_row_first":              # the ghost takes row 0 of its scale, face f row f + 1
            ar, dm, raw = np.roll(ar, 1), np.roll(dm, 1), np.roll(raw, 1)
            ei = np.where(ei == d["nf"], 0, ei + 1)
            if s == 0:
                node_bc = face_ptr[0]
        x[rows, 0], x[rows, 1], area_raw[rows] = ar, dm, raw
        eis.append(ei + face_ptr[s])
        attrs.append(_standardize(d["dist"]))
    for s in range(S - 1):
        pairs = intra_ref(sc[s]["c"], sc[s + 1]["xy"], sc[s + 1]["fn"])
        pairs = np.concatenate([pairs, [[sc[s + 1]["nf"]], [sc[s]["nf"]]]], 1)
        intra.append(pairs + np.array([[face_ptr[s + 1]], [face_ptr[s]]]))
    return dict(
        x=x, edge_index=np.concatenate(eis, 1).astype(np.int64),
        edge_attr=np.concatenate(attrs)[:, None].astype(np.float32),
        edge_ptr=np.cumsum([0] + [e.shape[1] for e in eis]).astype(np.int64), node_ptr=face_ptr.astype(np.int64),
        intra_mesh_edge_index=(np.concatenate(intra, 1) if intra else np.zeros((2, 0))).astype(np.int64),
        intra_edge_ptr=np.cumsum([0] + [p.shape[1] for p in intra]).astype(np.int64),
        BC=np.asarray(hydrograph_bc(T, previous_t) if BC is None else BC, np.float32),
        node_BC=np.array([node_bc], np.int32), area=area_raw.astype(np.float32),
        edge_BC_length=np.array([d["bc_edge_len"] for d in sc], np.float32),
        bc_face=[d["bc_face"] for d in sc], orphans=orphans, childless=childless)


GRAPH_ARRAYS = ("x", "edge_index", "edge_attr", "edge_ptr", "node_ptr", "intra_mesh_edge_index", "intra_edge_ptr",
                "BC", "node_BC", "area", "edge_BC_length")


# ----------------------------------------------------------------------------- planted meshes
def two_tri():
    xy = np.array([[0, 0], [8, 0], [8, 8], [0, 8]], np.float64)
    return xy, np.array([[0, 1, 2], [2, 3, 0]], np.int32)


def fan(n):
    """n faces round vertex 0 (a closed fan: every rim vertex on the unit circle's polygon)."""
    t = 2 * np.pi * np.arange(n) / n
    xy = np.concatenate([[[0.0, 0.0]], np.stack([np.cos(t), np.sin(t)], 1)])
    return xy, np.array([[0, 1 + k, 1 + (k + 1) % n] for k in range(n)], np.int32)


def mixed(xy, faces):
    """Every second face in the other orientation."""
    faces = faces.copy()
    faces[1::2] = faces[1::2][:, [0, 2, 1]]
    return xy, faces


def permuted(xy, faces, seed):
    """Face ids and vertex ids permuted, and three vertices that no face uses."""
    rng = np.random.default_rng(seed)
    V = xy.shape[0] + 3
    new_of_old = rng.permutation(V)[:xy.shape[0]]
    out = np.full((V, 2), 77.0)
    out[new_of_old] = xy
    return out, new_of_old[faces][rng.permutation(len(faces))].astype(np.int32)


def _dual_cases():
    c = {"one_triangle": rc.tri((0, 1, 2)), "one_triangle_cw": rc.tri((0, 2, 1)), "two_triangles": two_tri(),
         "hex_fan": rc.hex_fan(), "fan40": fan(40), "huge_and_tiny": rc.huge_and_tiny()}
    for n in range(1, 10):
        c[f"squares{n}"] = rc.squares(n)
    c["mixed_orientation"] = mixed(*rc.squares(5))
    c["permuted_unused"] = permuted(*rc.squares(6), seed=3)
    c["generator"] = multiscale_geometry(3, 3, 1)[0]
    return c


DUAL_CASES = _dual_cases()


def probe_points(xy, faces):
    """Vertices, edge midpoints, centroids, both float64 neighbours of each, points outside the
    hull and far outside, NaN, +-inf and -0.0."""
    xy = np.asarray(xy, np.float64)
    tri = xy[np.asarray(faces)]
    mids = 0.5 * (tri + tri[:, [1, 2, 0]])
    base = np.concatenate([xy, mids.reshape(-1, 2), tri.mean(1)])
    near = [base]
    for sx in (-np.inf, np.inf):
        for sy in (-np.inf, np.inf):
            near.append(np.stack([np.nextafter(base[:, 0], sx), np.nextafter(base[:, 1], sy)], 1))
        near.append(np.stack([np.nextafter(base[:, 0], sx), base[:, 1]], 1))
        near.append(np.stack([base[:, 0], np.nextafter(base[:, 1], sx)], 1))
    lo, hi = xy.min(0), xy.max(0)
    span = (hi - lo).max()
    odd = np.array([[lo[0] - 0.25 * span, lo[1]], [hi[0], hi[1] + 0.25 * span], [lo[0] - 1e6 * span, lo[1] - 1e6 * span],
                    [1e300, -1e300], [np.nan, lo[1]], [lo[0], np.nan], [np.nan, np.nan], [np.inf, lo[1]],
                    [lo[0], -np.inf], [-np.inf, np.inf], [-0.0, -0.0], [-0.0, 0.0], [0.0, -0.0]])
    return np.ascontiguousarray(np.concatenate(near + [odd]))


def _locate_cases():
    """name -> (xy, faces, face_row)."""
    c = {"tri_ccw": (*rc.tri((0, 1, 2)), None), "tri_cw": (*rc.tri((0, 2, 1)), None), "hex_fan": (*rc.hex_fan(), None),
         "squares5": (*rc.squares(5), None), "mixed_orientation": (*mixed(*rc.squares(4)), None),
         "huge_and_tiny": (*rc.huge_and_tiny(), None)}
    for name in ("overlap", "zero_area_first", "novalue_covers", "permuted_rows", "sliver", "utm_offset"):
        c[name] = rc.CASES[name][:3]
    return c


LOCATE_CASES = _locate_cases()


# ----------------------------------------------------------------------------- multiscale cases
def generator_inputs(n, S, seed):
    """-> (scales, bc_xy, finest dem) of make_multiscale_mesh(n, S, seed): the generator's own BC
    point and its finest DEM, drawn as it draws them."""
    scales = multiscale_geometry(n, S, seed)
    rng = np.random.default_rng(seed)
    _coarse_triangulation(n, rng)                    # the generator's first draws: the jitter
    xy, fn = scales[0]
    c = xy[fn].mean(1)
    dem = _smooth_dem(c[:, 0], c[:, 1], rng)
    side = n * 2 ** (S - 1)
    return scales, (0.0, (side // 2 + 0.5) * 1000.0 / side), dem


def independent_scales(ns, seed, size=1000.0, fine_size=None):
    """Independent triangulations of the same square, finest first: not nested.  ``fine_size``: the
    finest mesh covers a larger square, so it overhangs the coarser hulls."""
    out = []
    for k, n in enumerate(ns):
        xy, tris = _coarse_triangulation(n, np.random.default_rng([seed, k]), 0.25,
                                         fine_size if (k == 0 and fine_size) else size)
        out.append((np.ascontiguousarray(xy), np.ascontiguousarray(tris, np.int32)))
    return out


def dem_of(scale, seed):
    xy, fn = scale
    c = xy[fn].mean(1)
    return _smooth_dem(c[:, 0], c[:, 1], np.random.default_rng([seed, 99]))


def _graph_cases():
    """name -> (scales, bc_xy, dem)."""
    c = {}
    s = independent_scales((12, 6, 3), 5)
    c["non_nested"] = (s, (0.0, 520.0), dem_of(s[0], 5))
    s = independent_scales((12, 5), 6)
    c["bc_drift"] = (s, (0.0, 401.0), dem_of(s[0], 6))  # the finest midpoint (375) and the point straddle y = 400
    s = independent_scales((12, 6, 3), 7, fine_size=1100.0)
    c["overhang"] = (s, (0.0, 520.0), dem_of(s[0], 7))
    s = independent_scales((3, 6), 8)                  # coarser "fine" scale: childless coarse faces
    c["childless"] = (s, (0.0, 520.0), dem_of(s[0], 8))
    c["generator_tiny"] = generator_inputs(2, 4, 0)
    return c


GRAPH_CASES = _graph_cases()
