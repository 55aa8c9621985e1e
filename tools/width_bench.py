"""What a padded hidden width costs: the zenodo4 mesh, seeded K4 models at F = 50 and F = 64.

Three paths of the same 48-step rollout, timed the way bench.py times its workload (warm-up
rollouts, then repeated timed rollouts ending in a device synchronise; here one sample per
rollout and their median, the three paths alternating inside every repeat so that drift of the
box hits them alike):

  hip_f50    the HIP engine at F = 50 (rows zero-padded to 64, the NT = 4 kernels)
  hip_f64    the HIP engine at F = 64 (what F = 50 is expected to cost)
  torch_f50  engine='torch' at F = 50: the ATen path engine='auto' took for this width before
             the engine accepted it

    python tools/width_bench.py [--T 48] [--reps 20] [--warmup 3] [--torch-reps 5] [--out FILE]

Prints one JSON line (medians, raw samples in ms, parity of the two F = 50 paths) and writes
it to --out if given.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mswe-gnn_amd")]


def build(F, T):
    from models.gnn import MSGNN
    from mswegnn.mesh import make_multiscale_mesh, mesh_config
    g = make_multiscale_mesh(**mesh_config("zenodo4"), T=T)
    m = MSGNN(num_node_features=8, num_edge_features=1, num_scales=4, hid_features=F, K=4, mlp_layers=3,
              seed=666, learned_residuals=True, mlp_activation="prelu", gnn_activation="tanh", edge_mlp=True,
              normalize=True, with_filter_matrix=True, with_gradient=True, with_WL=True, learned_pooling=False,
              skip_connections=True, previous_t=3)
    return g, m.eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=48)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-reps", type=int, default=5, help="timed rollouts of the torch path (seconds each)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("width_bench needs a GPU")
    import copy

    from mswegnn import _lib
    from mswegnn.engine import plan_for
    dev = torch.device("cuda", 0)
    T = a.T
    paths, outs = {}, {}
    g50, m50 = build(50, T)
    g64, m64 = build(64, T)
    gd = g50.to(dev)  # one mesh for all three
    for name, m, engine in (("hip_f50", m50, "hip"), ("hip_f64", m64, "hip"), ("torch_f50", copy.deepcopy(m50), "torch")):
        m = m.to(dev)
        m.engine = engine
        paths[name] = m
    plans = {k: plan_for(paths[k], gd) for k in ("hip_f50", "hip_f64")}
    bufs = {k: torch.empty(gd.num_nodes, 2, T, device=dev) for k in plans}

    def run(name):
        if name in plans:
            return plans[name].rollout(gd.x, gd.BC, gd.node_BC, gd.type_BC, T, out=bufs[name])
        return paths[name].rollout(gd, T)

    def timed(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = run(name)
        torch.cuda.synchronize()
        outs[name] = r
        return (time.perf_counter() - t0) * 1e3

    for name in paths:
        for _ in range(a.warmup if name in plans else 1):
            timed(name)
    ref = outs["torch_f50"].clone()
    samples = {k: [] for k in paths}
    for i in range(a.reps):
        for name in paths:
            if name in plans or i < a.torch_reps:
                samples[name].append(timed(name))
    den = ref.abs().amax(dim=(0, 1))
    den = torch.where(den > 0, den, torch.ones_like(den))  # an all-dry step: absolute error
    err = float(((outs["hip_f50"] - ref).abs().amax(dim=(0, 1)) / den).max())
    n0 = int(g50.node_ptr[1])
    med = {k: statistics.median(v) for k, v in samples.items()}
    st = {k: plans[k].stats() for k in plans}
    res = {
        "tool": "width_bench", "mesh": "zenodo4", "fine_nodes": n0, "all_nodes": int(gd.num_nodes), "T": T, "K": 4,
        "weights": "seeded-init(seed=666)", "device": torch.cuda.get_device_name(0),
        "warmup": a.warmup, "reps": {k: len(v) for k, v in samples.items()},
        "median_ms_per_rollout": med,
        "min_ms_per_rollout": {k: min(v) for k, v in samples.items()},
        "fine_node_steps_per_s": {k: n0 * T / (med[k] * 1e-3) for k in med},
        "f50_over_f64": med["hip_f50"] / med["hip_f64"],
        "torch_f50_over_hip_f50": med["torch_f50"] / med["hip_f50"],
        "hip_f50_vs_torch_f50_max_rel_per_step": err,
        "plan": {k: {f: st[k][f] for f in ("hid_features", "padded_features", "kernels_per_step", "device_bytes")}
                 for k in st},
        "lib_sha256": _lib.lib_info()["sha256"],
        "samples_ms": samples,
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
