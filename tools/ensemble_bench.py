"""The ensemble kernels against the same products composed from torch ops on the same device.

    python tools/ensemble_bench.py [--out profiles/ensemble/bench.json] [--quick]

Seeded synthetic rollouts of 16 members, thresholds 0.05 / 0.3:
  * 16 x 10,369 cells, T = 48: zenodo4 x 16 members, laid out as its batch is (3,405 coarse rows
    after every member's cells).  32 MB of depths: it sits in the caches, and the figure is
    launch-bound, not a bandwidth;
  * [16 x 65,536, 2, 100]: 0.84 GB, the HBM-sized case of the sibling benches.
Kernel A (msw_ensemble_steps_update, every output) runs against its torch composition over the
[M, n, T] view of the depths: ``(h > thr).sum(0)`` per threshold, ``mean``, ``amin``, ``amax``.
Kernel B (msw_ensemble_maps on each member's peak depth and first wet step, p10 / p50 / p90) runs
against ``torch.sort`` plus indexing, counts and a mean.  The outputs of the two sides are compared
before timing: everything exactly, the torch means (fp32 sums in torch's own order) within
M 2^-24 max|h|.
Timing: warm-up, then 9 repeats in which the two sides alternate, each repeat a window of calls
under a host clock that ends in a device synchronise; medians.  Algorithmic bytes -- kernel A reads
M n T 4 and writes n T (4 n_thr + 12); kernel B reads 2 M n 4 and writes n (4 n_thr + 8 + 8 n_ranks)
-- over the median time, also as a fraction of the ~6.3 TB/s achievable HBM rate.
Needs a GPU; there is no fallback.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mswe-gnn_amd"))

from mswegnn import _lib  # noqa: E402
from mswegnn.ensemble import STEP_NAMES, EnsembleSteps, quantile_rank, steps_launch  # noqa: E402
from mswegnn.floodmaps import flood_maps  # noqa: E402

THR = (0.05, 0.3)
PROBS = (0.1, 0.5, 0.9)
HBM_ACHIEVABLE = 6.3e12
REPEATS = 9


def synthetic(n, T, dev, seed=0):
    """A flood front per row: dry until a seeded arrival step, then rising with seeded noise;
    q = h * u with both signs (tools/floodmaps_bench.py uses the same rollouts)."""
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


def window(fn, calls):
    """Seconds per call of ``calls`` calls under a host clock that ends in a device synchronise."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def alternate(kernel, composed, calls_kernel, calls_torch):
    """Medians (and min, max) of REPEATS windows per side, the sides alternating."""
    for _ in range(3):
        kernel()
        composed()
    tk, tt = [], []
    for _ in range(REPEATS):
        tk.append(window(kernel, calls_kernel))
        tt.append(window(composed, calls_torch))
    return (statistics.median(tk), min(tk), max(tk)), (statistics.median(tt), min(tt), max(tt))


def record(tk, tt, nbytes, calls_kernel, calls_torch):
    return {"algorithmic_bytes": nbytes, "repeats": REPEATS,
            "kernel_us": tk[0] * 1e6, "kernel_us_min_max": [tk[1] * 1e6, tk[2] * 1e6], "kernel_calls_per_window": calls_kernel,
            "torch_us": tt[0] * 1e6, "torch_us_min_max": [tt[1] * 1e6, tt[2] * 1e6], "torch_calls_per_window": calls_torch,
            "speedup_vs_torch": tt[0] / tk[0], "kernel_beats_torch": bool(tk[0] < tt[0]),
            "kernel_bytes_per_s": nbytes / tk[0], "fraction_of_hbm_achievable_6p3TBs": nbytes / tk[0] / HBM_ACHIEVABLE}


def bench(M, n, gap, T, dev, calls, launch_bound):
    N = M * (n + gap)
    pred = synthetic(N, T, dev)
    ranges = [(m * (n + gap), m * (n + gap) + n) for m in range(M)]
    lib = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    thr = (C.c_float * 2)(*THR)
    view = pred.view(M, n + gap, 2, T)[:, :n, 0, :]          # [M, n, T], strided: what a user holds

    # ---- kernel A
    es = EnsembleSteps(ranges, T, THR, device=dev)
    o = _lib.MswEnsembleStepsOut(**{k: es.arrays[k].data_ptr() for k in STEP_NAMES})
    row0 = (C.c_int64 * M)(*[s for s, _ in ranges])

    def steps_kernel():
        rc = lib.msw_ensemble_steps_update(C.c_void_p(pred.data_ptr()), T, 0, T, row0, M, n, thr, 2, T, 0, C.byref(o), st)
        if rc:
            _lib.check(rc)

    def steps_torch():
        return {"wet_members": torch.stack([(view > t).sum(0).to(torch.int32) for t in THR]),
                "h_mean": view.mean(0), "h_min": view.amin(0), "h_max": view.amax(0)}

    steps_kernel()
    ref = steps_torch()
    torch.cuda.synchronize()
    same = {k: bool(torch.equal(es.arrays[k], ref[k])) for k in ("wet_members", "h_min", "h_max")}
    same["h_mean_within_M_2^-24_max"] = bool(((es.arrays["h_mean"] - ref["h_mean"]).abs()
                                              <= M * 2.0 ** -24 * ref["h_max"]).all())
    del ref
    tk, tt = alternate(steps_kernel, steps_torch, calls[0], calls[1])
    g, c, it = steps_launch(n, M, T)
    a = {"launch": {"grid": g, "cells_per_wg": c, "iters": it}, "kernel_vs_torch": same,
         **record(tk, tt, M * n * T * 4 + n * T * (4 * len(THR) + 12), calls[0], calls[1])}

    # ---- kernel B on the members' flood maps
    maps = flood_maps(pred, ranges=ranges, thresholds=THR, want=("h_max", "first_wet"))
    values = torch.stack([m["h_max"] for m in maps])
    steps = torch.stack([m["first_wet"][THR[0]] for m in maps])
    ranks = [quantile_rank(p, M) for p in PROBS]
    out = {"exceed_members": torch.empty(2, n, dtype=torch.int32, device=dev), "mean": torch.empty(n, device=dev),
           "rank_values": torch.empty(3, n, device=dev), "members_with_step": torch.empty(n, dtype=torch.int32, device=dev),
           "rank_steps": torch.empty(3, n, dtype=torch.int32, device=dev)}
    ob = _lib.MswEnsembleMapsOut(**{k: v.data_ptr() for k, v in out.items()})
    rk = (C.c_int32 * 3)(*ranks)
    idx = torch.tensor(ranks, device=dev)
    big = torch.iinfo(torch.int32).max

    def maps_kernel():
        rc = lib.msw_ensemble_maps(C.c_void_p(values.data_ptr()), C.c_void_p(steps.data_ptr()), M, n, thr, 2, rk, 3,
                                   C.byref(ob), st)
        if rc:
            _lib.check(rc)

    def maps_torch():
        key = torch.where(steps < 0, big, steps)
        sel = torch.sort(key, dim=0, stable=True).values[idx]
        return {"exceed_members": torch.stack([(values > t).sum(0).to(torch.int32) for t in THR]),
                "mean": values.mean(0), "rank_values": torch.sort(values, dim=0, stable=True).values[idx],
                "members_with_step": (steps >= 0).sum(0).to(torch.int32), "rank_steps": torch.where(sel == big, -1, sel)}

    maps_kernel()
    ref = maps_torch()
    torch.cuda.synchronize()
    same = {k: bool(torch.equal(out[k], ref[k].to(out[k].dtype))) for k in out if k != "mean"}
    same["mean_within_M_2^-24_max"] = bool(((out["mean"] - ref["mean"]).abs() <= M * 2.0 ** -24 * values.amax(0)).all())
    del ref
    tk, tt = alternate(maps_kernel, maps_torch, calls[2], calls[3])
    b = {"probs": list(PROBS), "ranks": ranks, "kernel_vs_torch": same,
         **record(tk, tt, 2 * M * n * 4 + n * (4 * len(THR) + 8 + 8 * len(ranks)), calls[2], calls[3])}
    return {"shape": [N, 2, T], "members": M, "cells": n, "rows_between_members": gap, "thresholds": list(THR),
            "launch_bound": launch_bound, "steps": a, "maps": b}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble", "bench.json"))
    ap.add_argument("--quick", action="store_true", help="fewer calls per timing window")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_bench needs a GPU")
    dev = torch.device("cuda:0")
    q = 4 if a.quick else 1
    res = {"device": torch.cuda.get_device_name(0), "lib": _lib.lib_info()["sha256"],
           "sizes": [bench(16, 10369, 3405, 48, dev, (2000 // q, 400 // q, 2000 // q, 400 // q), True),
                     bench(16, 65536, 0, 100, dev, (100 // q, 20 // q, 1000 // q, 200 // q), False)]}
    res["every_kernel_beats_torch"] = all(s[k]["kernel_beats_torch"] for s in res["sizes"] for k in ("steps", "maps"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
