"""What a mesh's numbering costs the rollout, and what the locality order (mswegnn.locality,
msw_plan_create_ordered) gives back; and what building the order costs.

    python tools/locality_bench.py [--out profiles/locality/bench.json] [--quick]

  * rollout: one mesh under four numberings -- (1) the generator's, (2) a seeded random renumbering
    with no order (what a plan does with such a mesh unasked: the baseline), (3) that renumbering
    with the Hilbert ``row_order``, (4) the generator's numbering with the Hilbert order (the cost
    where the numbering was already good) -- on zenodo4 (T = 48) and on the hbm1m mesh (T = 8), both
    built by ``graph_from_meshes`` so that rows have coordinates.  One plan each, one warm-up
    rollout, then 7 rounds that run the four one after the other (alternating windows), a host clock
    that ends in a device synchronise; medians with min and max, per step.  The outputs of (2) and
    (3), and of (1) and (4), are asserted bit-equal; ``block_span`` of each layout stands beside it.
  * order: ``msw_locality_order`` on 131,072, 2^20 and 2^22 uniform points, one segment: the key
    kernel and the sort between device events (5 calls, medians), the host clock round the call;
    beside numpy's stable argsort of the same keys on the host and ``torch.sort(stable=True)`` of
    them on the device (yardsticks, not thresholds).
``--quick``: zenodo4 only and the smallest order size, for a rehearsal.  Needs a GPU; no fallback.
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

from models.gnn import MSGNN  # noqa: E402
from mswegnn import locality as loc  # noqa: E402
from mswegnn.engine import EnginePlan  # noqa: E402
from mswegnn.mesh import Graph, irregularize, mesh_config, multiscale_geometry, wet_state  # noqa: E402
from mswegnn.meshgraph import graph_from_meshes  # noqa: E402

ROUNDS = 7


def med(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "repeats": len(v)}


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def build_mesh(name, T, dev):
    cfg = mesh_config(name)
    geo = multiscale_geometry(cfg["n_coarse"], cfg["num_scales"], 0)
    xy, fn = geo[0]
    c = xy[fn].mean(1)
    mg = graph_from_meshes(geo, (0.0, 500.0), 0.004 * c[:, 0] + 0.002 * c[:, 1], T=T, device=dev)
    return wet_state(mg.graph, seed=1, all_wet=True), mg.row_xy, cfg["num_scales"]


def bench_rollout(name, T, dev):
    g, xy, S = build_mesh(name, T, dev)
    gr, old = irregularize(g, 9, move=0.0, orphan=0.0, delete=0.0, permute=True)  # a renumbering, nothing else
    xyr = xy[old]
    model = MSGNN(num_node_features=8, num_edge_features=1, num_scales=S, hid_features=32, K=4, mlp_layers=3,
                  seed=666, learned_residuals=True, mlp_activation="prelu", gnn_activation="tanh", edge_mlp=True,
                  normalize=True, with_filter_matrix=True, with_gradient=True, with_WL=True, learned_pooling=False,
                  skip_connections=True, previous_t=3).eval().to(dev)
    build = {}
    variants = {}
    for key, graph, pts, ordered in (("generator", g, xy, False), ("random", gr, xyr, False),
                                     ("random_hilbert", gr, xyr, True), ("generator_hilbert", g, xy, True)):
        gd = graph.to(dev)
        order = None
        if ordered:
            stats = {}
            build[key], order = clocked(lambda: loc.row_order(graph, pts.to(dev), stats=stats))
            build[key] = {"row_order_seconds": build[key], **stats}
            gd.row_order = order
        t_plan, plan = clocked(lambda: EnginePlan(model, gd, dev))
        layout = plan.row_layout()
        variants[key] = dict(plan=plan, g=gd, plan_seconds=t_plan,
                             block_span=loc.block_span(graph, layout[layout >= 0].astype(np.int64)))
    outs = {}
    for key, v in variants.items():  # warm-up, and the outputs compared
        gd = v["g"]
        outs[key] = v["plan"].rollout(gd.x, gd.BC, gd.node_BC, gd.type_BC, T)
    torch.cuda.synchronize()
    equal = {"random_vs_random_hilbert": bool(torch.equal(outs["random"], outs["random_hilbert"])),
             "generator_vs_generator_hilbert": bool(torch.equal(outs["generator"], outs["generator_hilbert"]))}
    assert all(equal.values()), equal
    assert float(outs["generator"].abs().max()) > 0
    back = torch.empty_like(outs["random"])
    # informative only: irregularize's canonical edge order sorts each destination's in-edges by the NEW
    # numbers, so the renumbered mesh adds them in another order and need not give the generator's bits
    back[torch.from_numpy(old).to(dev)] = outs["random"]
    equal["random_mapped_back_vs_generator"] = bool(torch.equal(back, outs["generator"]))
    times = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for key, v in variants.items():
            gd = v["g"]
            out = outs[key]
            t, _ = clocked(lambda: v["plan"].rollout(gd.x, gd.BC, gd.node_BC, gd.type_BC, T, out=out))
            times[key].append(t / T)
    res = {"mesh": name, "num_nodes": g.num_nodes, "num_edges": int(g.edge_index.shape[1]), "scales": S, "T": T,
           "bit_equal": equal, "order_build": build, "seconds_per_step": {}}
    base = statistics.median(times["random"])
    for key, v in variants.items():
        m = med(times[key])
        res["seconds_per_step"][key] = {**m, "block_span_finest": v["block_span"], "plan_seconds": v["plan_seconds"],
                                        "vs_random": m["median"] / base}
        v["plan"].close()
    return res


def bench_order(n, dev):
    rng = np.random.default_rng(n)
    xy = torch.from_numpy(rng.random((n, 2))).to(dev)

    G = Graph(x=torch.empty(n, 1))  # a graph of one segment
    keys_us, sort_us, wall, scratch = [], [], [], 0
    loc.row_order(G, xy)
    for _ in range(5):
        stats = {}
        t, order = clocked(lambda: loc.row_order(G, xy, stats=stats))
        keys_us.append(stats["keys_us"]), sort_us.append(stats["sort_us"]), wall.append(t)
        scratch = stats["scratch_bytes"]
    keys = loc.hilbert_keys(xy, (0.0, 0.0, 1.0))
    hk = keys.cpu().numpy().astype(np.uint32)
    t0 = time.perf_counter()
    want = np.argsort(hk, kind="stable")
    host = time.perf_counter() - t0
    box = loc.bounding_square(xy)
    same = bool(np.array_equal(np.argsort(loc.hilbert_keys(xy, box).cpu().numpy(), kind="stable"), order.numpy()))
    assert same
    torch.sort(keys, stable=True)
    ts = [clocked(lambda: torch.sort(keys, stable=True))[0] for _ in range(5)]
    return {"rows": n, "launch": dict(zip(("grid", "items_per_wg", "iters"), loc.locality_launch(n))),
            "keys_us": med(keys_us), "sort_us": med(sort_us), "call_seconds_incl_copy_back": med(wall),
            "scratch_bytes": scratch, "equals_numpy_stable_argsort": same,
            "numpy_stable_argsort_seconds": host, "numpy_rows": int(len(want)),
            "torch_sort_stable_int64_seconds": med(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "locality", "bench.json"))
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "rollout": [], "order": []}
    for n in ([131072] if a.quick else [131072, 2 ** 20, 2 ** 22]):
        res["order"].append(bench_order(n, dev))
        print(json.dumps(res["order"][-1]), flush=True)
    for name, T in ([("zenodo4", 48)] if a.quick else [("zenodo4", 48), ("hbm1m", 8)]):
        res["rollout"].append(bench_rollout(name, T, dev))
        print(json.dumps(res["rollout"][-1]), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:  # rewritten after every mesh, so that partial results survive
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
