"""Cases and numpy restatements for the locality order (csrc/locality.hip, mswegnn/locality.py),
shared by tests/test_locality.py (CPU) and tests/test_gpu_locality.py.

hilbert_keys_ref is the definition of k_hilbert_keys' output, bit for bit: the quantisation is a
sequence of separate float64 operations and the curve an integer bit loop.  order_ref is the
definition of the sort's: a stable argsort per segment.
"""
import numpy as np

LAST_KEY = 0xFFFFFFFF


def hilbert_index_ref(ix, iy, order=16):
    """Index of the cells (ix, iy) on the Hilbert curve with 2^order cells a side -> int64."""
    x, y = np.asarray(ix, np.int64).copy(), np.asarray(iy, np.int64).copy()
    d = np.zeros_like(x)
    top = (1 << order) - 1
    s = 1 << (order - 1)
    while s > 0:
        rx = ((x & s) != 0).astype(np.int64)
        ry = ((y & s) != 0).astype(np.int64)
        d += s * s * ((3 * rx) ^ ry)
        turn = ry == 0
        mirror = turn & (rx == 1)
        x[mirror], y[mirror] = top - x[mirror], top - y[mirror]
        x[turn], y[turn] = y[turn].copy(), x[turn].copy()
        s >>= 1
    return d


def _cell_ref(v, lo, sc):
    with np.errstate(all="ignore"):
        f = (v - np.float64(lo)) * sc
        out = np.zeros(f.shape, np.int64)
        mid = (f >= 0) & (f < 65536.0)
        out[mid] = np.floor(f[mid]).astype(np.int64)
        out[f >= 65536.0] = 65535
    return out


def hilbert_keys_ref(xy, box):
    """uint32 [n]: the key of every row of xy float64 [n, 2] in box = (x0, y0, side)."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    x0, y0, side = box
    sc = np.float64(65536.0) / np.float64(side)
    keys = hilbert_index_ref(_cell_ref(xy[:, 0], x0, sc), _cell_ref(xy[:, 1], y0, sc))
    keys[~np.isfinite(xy).all(1)] = LAST_KEY
    return keys.astype(np.uint32)


def order_ref(keys, seg_ptr=None):
    """int64 [n]: inside each segment the rows by ascending key, ties to the lower row."""
    keys = np.asarray(keys)
    seg_ptr = [0, len(keys)] if seg_ptr is None else seg_ptr
    out = np.empty(len(keys), np.int64)
    for a, b in zip(seg_ptr[:-1], seg_ptr[1:]):
        out[a:b] = a + np.argsort(keys[a:b], kind="stable")
    return out


# ----------------------------------------------------------------------------- key cases
def _edge_points(box):
    """Cell boundaries and their float64 neighbours, both ends of the box, points outside it (they
    clamp), -0.0, NaN and +-inf (the last key)."""
    x0, y0, side = box
    h = side / 65536.0
    xs = [x0, x0 + h, x0 + 7 * h, x0 + 32768 * h, x0 + 65535 * h, x0 + side, x0 - side, x0 + 3 * side,
          x0 + 0.5 * h, x0 + 65535.5 * h, -0.0, 0.0]
    xs += [np.nextafter(v, -np.inf) for v in xs[:6]] + [np.nextafter(v, np.inf) for v in xs[:6]]
    pts = [(a, b) for a in xs for b in (y0, y0 + 0.25 * side, y0 + side, -0.0)]
    pts += [(b, a) for a, b in pts]
    bad = [np.nan, np.inf, -np.inf]
    pts += [(v, y0 + 0.5 * side) for v in bad] + [(x0 + 0.5 * side, v) for v in bad] + [(np.nan, np.inf)]
    return np.array(pts, np.float64)


def _key_cases():
    rng = np.random.default_rng(11)
    unit = (0.0, 0.0, 1.0)
    odd = (-317.25, 1200.5, 1000.0 / 3.0)
    cases = {
        "uniform_unit": (rng.random((700, 2)), unit),
        "uniform_odd_box": (np.array(odd[:2]) + rng.random((700, 2)) * odd[2], odd),
        "edges_unit": (_edge_points(unit), unit),
        "edges_odd_box": (_edge_points(odd), odd),
        "one_cell": (np.full((130, 2), 0.5) + rng.random((130, 2)) * 2.0 ** -20, unit),
    }
    ii, jj = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    cases["cell_centres_32"] = (np.stack([ii.ravel() + 0.5, jj.ravel() + 0.5], 1) / 32.0, unit)
    return cases


KEY_CASES = _key_cases()


# ----------------------------------------------------------------------------- sort cases
def sort_keys(name, n, seed=3):
    """uint32 [n] keys of one named pattern."""
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.uint64)
    if name == "all_equal":
        k = np.full(n, 0x12345678, np.uint64)
    elif name == "ascending":
        k = i * 977
    elif name == "descending":
        k = (n - 1 - i) * 977
    elif name == "low_digit":
        k = 0xABCDEF00 + rng.integers(0, 256, n).astype(np.uint64)
    elif name == "high_digit":
        k = (rng.integers(0, 256, n).astype(np.uint64) << np.uint64(24)) + 0x00C0FFEE
    elif name == "every_digit":
        k = rng.permutation((i % 256) * 0x01010101)
    elif name == "three_values":
        k = np.array([5, 0x80000000, 0x00FF00FF], np.uint64)[rng.integers(0, 3, n)]
    elif name == "extremes":
        k = np.array([0, LAST_KEY], np.uint64)[rng.integers(0, 2, n)]
    else:
        assert name == "random"
        k = rng.integers(0, 2 ** 32, n).astype(np.uint64)
    return (k & np.uint64(LAST_KEY)).astype(np.uint32)


SORT_PATTERNS = ["all_equal", "ascending", "descending", "low_digit", "high_digit", "every_digit", "three_values",
                 "extremes", "random"]


# ----------------------------------------------------------------------------- meshes
def quadtree_graph(n_coarse=8, num_scales=4, seed=0, T=2):
    """(graph, row_xy) of the generator's mesh through graph_from_meshes (so that rows have
    coordinates)."""
    from mswegnn.mesh import multiscale_geometry
    from mswegnn.meshgraph import graph_from_meshes
    geo = multiscale_geometry(n_coarse, num_scales, seed)
    mg = graph_from_meshes(geo, (0.0, 500.0), np.zeros(geo[0][1].shape[0]), T=T)
    return mg.graph, mg.row_xy


def renumbered(graph, row_xy, seed):
    """The graph with the faces of every scale randomly renumbered (ghosts stay last; structure
    untouched) -> (graph, row_xy, old_of_new)."""
    from mswegnn.mesh import irregularize
    g, old = irregularize(graph, seed, move=0.0, orphan=0.0, delete=0.0, permute=True)
    return g, row_xy[old], old
