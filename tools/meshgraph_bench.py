"""The mesh-graph kernels and the builder on the hbm1m geometry (config 5: 1,002,528 finest faces,
three scales), each beside what the tree had before.

    python tools/meshgraph_bench.py [--out profiles/meshgraph/bench.json] [--quick]

  * locate: the 1,002,528 finest centroids located in the 250,632 faces of the next scale by
    k_locate_points, in mesh order and shuffled; warm-up, then 9 windows of calls under a host
    clock that ends in a device synchronise, medians with min and max, as points per second.  The
    rows are checked first: every fine face's parent is ``f // 4`` on this geometry.  Beside it,
    k_raster_locate over the same 250,632 faces onto a 1,001 x 1,001 grid covering the mesh
    (``locate_us`` of 5 handles, device events): pixels per second at the same face count.
  * dual: ``msw_mesh_dual_create`` on the finest scale, 5 handles: the host clock round all of
    create, its host part (checks, vertex CSR, prefix sum) and the two kernels between device
    events; beside ``mswegnn.mesh._dual_graph`` on the same triangles (once: Python dicts).
  * build: ``graph_from_meshes`` end to end (3 runs, host clock, device synchronised) beside
    ``make_multiscale_mesh(**mesh_config('hbm1m'))`` (once), the tree's only builder before; the
    two graphs' index arrays are compared with ``torch.equal`` and the float columns bit for bit
    or within 1 fp32 ulp (``edge_attr``).  The geometry itself (``multiscale_geometry``) is input
    to both and timed apart.
``--quick`` runs the same code on zenodo3 (10,368 finest faces), for a rehearsal.  Needs a GPU;
there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mswe-gnn_amd"))

from mswegnn import _lib  # noqa: E402
from mswegnn.mesh import (_coarse_triangulation, _dual_graph, _smooth_dem, make_multiscale_mesh, mesh_config,  # noqa: E402
                          multiscale_geometry)
from mswegnn.meshgraph import DualGraph, PointLocator, graph_from_meshes, locate_launch, mesh_dual_launch  # noqa: E402
from mswegnn.raster import RasterGrid, Rasterizer  # noqa: E402

REPEATS = 9


def med(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "repeats": len(v)}


def window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def bench_locate(scales, dev):
    (fxy, ffn), (cxy, cfn) = scales[0], scales[1]
    fine = DualGraph(fxy, ffn, device=dev)
    loc = PointLocator(cxy, cfn, device=dev)
    n = fine.num_faces
    ordered = fine.centroid.contiguous()
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(0)).to(dev)
    shuffled = ordered[perm].contiguous()
    parent = torch.arange(n, device=dev, dtype=torch.int32) // 4
    ok = bool(torch.equal(loc.locate(ordered), parent)) and bool(torch.equal(loc.locate(shuffled), parent[perm]))
    out = {"points": n, "faces": int(cfn.shape[0]), "rows_equal_generator_parents": ok,
           "launch": dict(zip(("grid", "points_per_wg", "iters"), locate_launch(n))), **loc.stats()}
    for name, pts in (("ordered", ordered), ("shuffled", shuffled)):
        for _ in range(3):
            loc.locate(pts)
        t = [window(lambda: loc.locate(pts), 20) for _ in range(REPEATS)]
        out[name] = {"seconds_per_call": med(t), "points_per_second": n / statistics.median(t)}
    side = int(round(n ** 0.5))
    lo, hi = cxy.min(0), cxy.max(0)
    grid = RasterGrid(lo[0], hi[1], (hi[0] - lo[0]) / (side - 1), -(hi[1] - lo[1]) / (side - 1), side, side)
    us = []
    for _ in range(5):
        r = Rasterizer(cxy, cfn, grid, device=dev)
        us.append(r.stats()["locate_us"])
        r.close()
    out["k_raster_locate_same_faces"] = {"grid": [side, side], "pixels": side * side, "locate_us": med(us),
                                         "pixels_per_second": side * side / (statistics.median(us) * 1e-6)}
    out["ordered_rate_over_raster_rate"] = out["ordered"]["points_per_second"] / \
        out["k_raster_locate_same_faces"]["pixels_per_second"]
    return out


def bench_dual(scales, dev):
    xy, fn = scales[0]
    DualGraph(xy, fn, device=dev)
    stats = []
    for _ in range(5):
        stats.append(DualGraph(xy, fn, device=dev).stats())
    t0 = time.perf_counter()
    pairs, _ = _dual_graph(fn.astype(np.int64))
    python_s = time.perf_counter() - t0
    d = DualGraph(xy, fn, device=dev)
    out = {"faces": int(fn.shape[0]), "edges": d.num_edges, "boundary": int(d.boundary.shape[0]),
           "launch": dict(zip(("grid", "faces_per_wg", "iters"), mesh_dual_launch(fn.shape[0]))),
           "longest_star": stats[0]["longest_star"], "device_bytes": stats[0]["device_bytes"],
           "edge_index_equals_dual_graph": bool(torch.equal(d.edge_index.cpu(), torch.from_numpy(pairs.reshape(2, -1)))),
           "create_seconds": med([s["create_seconds"] for s in stats]),
           "host_build_seconds": med([s["host_build_seconds"] for s in stats]),
           "k_mesh_faces_us": med([s["faces_us"] for s in stats]),
           "k_mesh_edges_us": med([s["edges_us"] for s in stats]),
           "python_dual_graph_seconds": python_s}
    out["create_over_python"] = python_s / out["create_seconds"]["median"]
    return out


def bench_build(cfg, scales, dev):
    n, S = cfg["n_coarse"], cfg["num_scales"]
    rng = np.random.default_rng(0)
    _coarse_triangulation(n, rng)
    xy, fn = scales[0]
    c = xy[fn].mean(1)
    dem = _smooth_dem(c[:, 0], c[:, 1], rng)
    side = n * 2 ** (S - 1)
    bc_xy = (0.0, (side // 2 + 0.5) * 1000.0 / side)
    t0 = time.perf_counter()
    g = make_multiscale_mesh(**cfg, T=6)
    generator_s = time.perf_counter() - t0
    graph_from_meshes(scales, bc_xy, dem, T=6, BC=g.BC, device=dev)
    runs = []
    for _ in range(3):
        s, m = clocked(lambda: graph_from_meshes(scales, bc_xy, dem, T=6, BC=g.BC, device=dev))
        runs.append(s)
    h = m.graph
    same = {k: bool(torch.equal(getattr(h, k), getattr(g, k)))
            for k in ("edge_index", "edge_ptr", "node_ptr", "intra_mesh_edge_index", "intra_edge_ptr", "node_BC", "area")}
    same["x"] = bool(torch.equal(h.x, g.x))
    a, b = h.edge_attr.numpy(), g.edge_attr.numpy()
    same["edge_attr_within_1_ulp"] = bool((np.abs(a.astype(np.float64) - b) <= np.spacing(np.maximum(np.abs(a), np.abs(b)))).all())
    same["edge_attr_bitwise"] = bool(torch.equal(h.edge_attr, g.edge_attr))
    return {"nodes": h.num_nodes, "edges": int(h.edge_index.shape[1]), "graph_from_meshes_seconds": med(runs),
            "make_multiscale_mesh_seconds": generator_s,
            "generator_over_builder": generator_s / statistics.median(runs), "equals_generator": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshgraph", "bench.json"))
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("meshgraph_bench needs a GPU")
    dev = torch.device("cuda:0")
    name = "zenodo3" if args.quick else "hbm1m"
    cfg = mesh_config(name)
    t0 = time.perf_counter()
    scales = multiscale_geometry(**cfg)
    res = {"device": torch.cuda.get_device_name(0), "lib": _lib.lib_info()["sha256"], "mesh": name,
           "faces_per_scale": [int(fn.shape[0]) for _, fn in scales],
           "geometry_seconds_python": time.perf_counter() - t0}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for key, fn in (("locate", lambda: bench_locate(scales, dev)), ("dual", lambda: bench_dual(scales, dev)),
                    ("build", lambda: bench_build(cfg, scales, dev))):
        res[key] = fn()
        print(key, json.dumps(res[key]), flush=True)
        with open(args.out, "w") as f:   # after every part: a later part's time limit loses nothing
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
