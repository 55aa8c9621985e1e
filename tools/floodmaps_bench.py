"""Flood-map kernel against the same maps composed from torch ops, and the cost of chunking a rollout.

    python tools/floodmaps_bench.py [--out profiles/floodmaps/bench.json] [--quick]

1. msw_flood_maps_update (every map, thresholds 0.05 / 0.3) on seeded synthetic rollouts
   [10,369, 2, 48] and [1,048,576, 2, 100] against the baseline: ``_maps_torch`` on the same
   device tensor (one [N, T] pass per torch op).  Timed with device events after warm-up; the
   outputs of the two are compared before timing.  Achieved bytes/s = (2 T 4 nrows + map bytes)
   / time, also as a fraction of the 8 TB/s HBM peak and of the ~6.3 TB/s achievable.  The small
   size (4 MB) sits in the Infinity Cache and its calls are launch-bound: only the large one
   says anything about HBM.
2. ``rollout_flood_maps(chunk=16)`` against ``model.rollout`` + one update, K4_F32 on the
   zenodo4 mesh at T = 48 (host clock around a device synchronise: it includes the host side of
   every msw_rollout call, whose prologue re-runs per chunk).
Needs a GPU; there is no fallback.
"""
import argparse
import ctypes as C
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
from mswegnn.floodmaps import MAP_NAMES, FloodMaps, _maps_torch, rollout_flood_maps  # noqa: E402

THR = (0.05, 0.3)
EPS = 0.01
HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12


def synthetic(n, T, dev, seed=0):
    """A flood front per row: dry until a seeded arrival step (about a quarter of the rows never
    exceed 0.05 m and about 60 % of the (row, step) pairs are dry; on fx_small_K4_F32_rollout48
    a third of the cells never exceed 0.05 m), then
    rising with seeded noise; q = h * u with both signs."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    arrival = torch.rand(n, 1, device=dev, generator=gen) * 1.25 * T
    depth = 0.2 + 1.8 * torch.rand(n, 1, device=dev, generator=gen)
    t = torch.arange(T, device=dev, dtype=torch.float32)[None]
    out = torch.empty(n, 2, T, device=dev)
    h = torch.clamp((t - arrival) / T, min=0.0) * depth
    h *= 0.75 + 0.5 * torch.rand(n, T, device=dev, generator=gen)
    out[:, 0] = h
    out[:, 1] = h * (torch.rand(n, T, device=dev, generator=gen) * 1.2 - 0.6)
    return out


def time_events(fn, iters, repeats=5):
    """Median over `repeats` windows of `iters` calls each, seconds per call."""
    per = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        per.append(a.elapsed_time(b) * 1e-3 / iters)
    return statistics.median(per), min(per), max(per)


def bench_kernel(n, T, dev, iters_kernel, iters_torch):
    pred = synthetic(n, T, dev)
    fm = FloodMaps(n, thresholds=THR, vel_eps=EPS, device=dev)
    m = _lib.MswFloodMaps(**{k: fm.maps[k].data_ptr() for k in MAP_NAMES})
    thr = (C.c_float * 2)(*THR)
    lib = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def kernel():
        rc = lib.msw_flood_maps_update(C.c_void_p(pred.data_ptr()), T, 0, T, 0, 0, n, thr, 2, EPS, 1, C.byref(m), st)
        if rc:
            _lib.check(rc)

    def composed():
        return _maps_torch(pred, THR, EPS)

    # the same call without vel_max / froude_max: what the two divisions and the square root cost
    m_nv = _lib.MswFloodMaps(**{k: fm.maps[k].data_ptr() for k in MAP_NAMES if k not in ("vel_max", "froude_max")})

    def kernel_no_velocity():
        rc = lib.msw_flood_maps_update(C.c_void_p(pred.data_ptr()), T, 0, T, 0, 0, n, thr, 2, EPS, 1, C.byref(m_nv), st)
        if rc:
            _lib.check(rc)

    kernel()
    ref = composed()
    torch.cuda.synchronize()
    equal = {k: bool(torch.equal(fm.maps[k], ref[k])) for k in MAP_NAMES}
    del ref
    for _ in range(3):
        kernel()
        kernel_no_velocity()
        composed()
    torch.cuda.synchronize()
    tk = time_events(kernel, iters_kernel)
    tn = time_events(kernel_no_velocity, iters_kernel)
    tt = time_events(composed, iters_torch)
    g, r, it = C.c_int32(), C.c_int32(), C.c_int32()
    lib.msw_flood_maps_launch(n, T, C.byref(g), C.byref(r), C.byref(it))
    nbytes = 2 * T * 4 * n + n * (6 + 3 * len(THR)) * 4
    return {"shape": [n, 2, T], "thresholds": list(THR), "launch": {"grid": g.value, "rows_per_wg": r.value, "iters": it.value},
            "equals_torch_composition": equal, "bytes": nbytes,
            "kernel_s": tk[0], "kernel_s_min_max": tk[1:], "kernel_calls_per_window": iters_kernel,
            "torch_s": tt[0], "torch_s_min_max": tt[1:], "torch_calls_per_window": iters_torch,
            "speedup_vs_torch": tt[0] / tk[0], "kernel_bytes_per_s": nbytes / tk[0],
            "fraction_of_hbm_peak_8TBs": nbytes / tk[0] / HBM_PEAK,
            "fraction_of_hbm_achievable_6p3TBs": nbytes / tk[0] / HBM_ACHIEVABLE,
            "kernel_no_velocity_s": tn[0], "kernel_no_velocity_bytes_per_s": (nbytes - 8 * n) / tn[0],
            "no_velocity_fraction_of_hbm_achievable_6p3TBs": (nbytes - 8 * n) / tn[0] / HBM_ACHIEVABLE}


def bench_chunking(dev, T=48, repeats=7):
    from models.gnn import MSGNN
    from mswegnn.mesh import make_multiscale_mesh, mesh_config
    z = np.load(os.path.join(ROOT, "tests", "golden", "weights_K4_F32.npz"))
    m = MSGNN(num_node_features=8, num_edge_features=1, num_scales=4, hid_features=32, K=4, mlp_layers=3, seed=666,
              learned_residuals=True, mlp_activation="prelu", gnn_activation="tanh", with_WL=True, previous_t=3)
    m.load_state_dict({k: torch.from_numpy(z[k]) for k in z.files}, strict=True)
    m = m.eval().to(dev)
    m.engine = "hip"
    g = make_multiscale_mesh(**mesh_config("zenodo4"), T=T).to(dev)

    def run(chunk):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = rollout_flood_maps(m, g, T, chunk=chunk, thresholds=THR)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res
    out = {"mesh": "zenodo4", "model": "K4_F32", "T": T, "rows": int(g.x.shape[0])}
    base = None
    for name, chunk in (("whole", None), ("chunk16", 16), ("chunk8", 8)):
        for _ in range(3):
            _, res = run(chunk)
        ts = []
        for _ in range(repeats):  # the variants are measured one after the other, each warmed up
            ts.append(run(chunk)[0])
        if base is None:
            base = res
        same = all(torch.equal(res[k], base[k]) for k in ("h_max", "t_h_max", "q_max", "vel_max", "froude_max"))
        out[name] = {"seconds": statistics.median(ts), "min_max": [min(ts), max(ts)], "maps_equal_whole": same}
    for k in ("chunk16", "chunk8"):
        out[k]["over_whole"] = out[k]["seconds"] / out["whole"]["seconds"]
        out[k]["extra_seconds_per_chunk"] = (out[k]["seconds"] - out["whole"]["seconds"]) / (T // int(k[5:]) - 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "floodmaps", "bench.json"))
    ap.add_argument("--quick", action="store_true", help="fewer calls per timing window")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("floodmaps_bench needs a GPU")
    dev = torch.device("cuda:0")
    q = 4 if a.quick else 1
    res = {"device": torch.cuda.get_device_name(0), "lib": _lib.lib_info()["sha256"],
           "kernel": [bench_kernel(10369, 48, dev, 4000 // q, 200 // q),
                      bench_kernel(1 << 20, 100, dev, 400 // q, 20 // q)],
           "chunking": bench_chunking(dev)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
