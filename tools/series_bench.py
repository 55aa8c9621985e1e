"""Zone-series kernel against the same series composed from torch ops on the same device.

    python tools/series_bench.py [--out profiles/series/bench.json] [--quick]

msw_zone_series_update (every series, thresholds 0.05 / 0.3, cell areas) on seeded synthetic
rollouts:
  * [1,048,576, 2, 100]: a seeded random 64-way partition of all rows plus 1,024 one-row gauges;
  * [10,369, 2, 48]: a seeded random partition into 8 zones.
The baseline is ``_series_torch`` on the device tensor (``index_select`` / ``index_add_`` /
``scatter_reduce_`` over the listed rows): the only way to get these series without the kernel.
Timed with device events after warm-up, medians of 5 windows; the outputs of the two are compared
before timing (counts and maxima exactly, the fp64 sums against 2 m 2^-53 sum|terms|).  Rate =
listed-row bytes (M * 2 * T * 4, M the list entries) / time, also as a fraction of the ~6.3 TB/s
achievable HBM rate.  The small size (4 MB) sits in the Infinity Cache: only the large one says
anything about HBM.  A third section times the large mesh at T = 128 and 64 (full 64-step tiles,
rows that start on a cache line) and with 64 zones of consecutive rows.
Needs a GPU; there is no fallback.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mswe-gnn_amd"))

from mswegnn import _lib  # noqa: E402
from mswegnn.series import SERIES_NAMES, ZoneSeries, Zones, _series_torch  # noqa: E402

THR = (0.05, 0.3)
HBM_ACHIEVABLE = 6.3e12


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


def compare(zs, ref, zones, pred, area):
    """-> exact equality of counts and maxima, and the largest |kernel - torch| / bound of the sums."""
    zone, rows = zones.lists(pred.device)
    m = zones.sizes.double().to(pred.device)[:, None]
    out = {k: bool(torch.equal(zs.series[k], ref[k])) for k in ("wet_cells", "h_max", "q_max")}
    abs_vol = _series_torch(pred.abs(), zone, rows, zones.num_zones, area, ())["volume"]
    for k, terms in (("volume", abs_vol), ("wet_area", ref["wet_area"])):
        bound = 2 * m * 2.0 ** -53 * terms
        err = (zs.series[k] - ref[k]).abs()
        ok = bound > 0
        out[k + "_error_over_bound"] = float((err[ok] / bound[ok]).max()) if bool(ok.any()) else 0.0
        out[k + "_within_bound"] = bool((err <= bound).all())
    return out


def bench(n, T, zones, dev, iters_kernel, iters_torch):
    pred = synthetic(n, T, dev)
    area = torch.rand(n, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 90 + 10
    zs = ZoneSeries(zones, T, area=area, thresholds=THR, device=dev)
    o = _lib.MswZoneSeries(**{k: zs.series[k].data_ptr() for k in SERIES_NAMES})
    thr = (C.c_float * 2)(*THR)
    lib = _lib.lib()
    h = zones.handle(dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    zone, rows = zones.lists(dev)

    def kernel():
        rc = lib.msw_zone_series_update(h, C.c_void_p(pred.data_ptr()), T, 0, T, C.c_void_p(area.data_ptr()), thr, 2,
                                        T, 0, C.byref(o), st)
        if rc:
            _lib.check(rc)

    def composed():
        return _series_torch(pred, zone, rows, zones.num_zones, area, THR)

    kernel()
    ref = composed()
    torch.cuda.synchronize()
    same = compare(zs, ref, zones, pred, area)
    del ref
    for _ in range(3):
        kernel()
        composed()
    torch.cuda.synchronize()
    tk = time_events(kernel, iters_kernel)
    tt = time_events(composed, iters_torch)
    M = int(zones.rows.numel())
    nbytes = M * 2 * T * 4
    g, u, it = zones.launch(T, dev)
    return {"shape": [n, 2, T], "zones": zones.num_zones, "listed_rows": M, "largest_zone": int(zones.sizes.max()),
            "thresholds": list(THR), "launch": {"grid": g, "units_per_wg": u, "iters": it},
            "kernel_vs_torch": same, "listed_row_bytes": nbytes,
            "kernel_us": tk[0] * 1e6, "kernel_us_min_max": [tk[1] * 1e6, tk[2] * 1e6], "kernel_calls_per_window": iters_kernel,
            "torch_us": tt[0] * 1e6, "torch_us_min_max": [tt[1] * 1e6, tt[2] * 1e6], "torch_calls_per_window": iters_torch,
            "speedup_vs_torch": tt[0] / tk[0], "kernel_bytes_per_s": nbytes / tk[0],
            "fraction_of_hbm_achievable_6p3TBs": nbytes / tk[0] / HBM_ACHIEVABLE}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "series", "bench.json"))
    ap.add_argument("--quick", action="store_true", help="fewer calls per timing window")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("series_bench needs a GPU")
    dev = torch.device("cuda:0")
    q = 4 if a.quick else 1
    gen = torch.Generator().manual_seed(0)
    n_big, n_small = 1 << 20, 10369
    big = Zones.from_labels(torch.randint(0, 64, (n_big,), generator=gen), num_zones=64) \
        + Zones.gauges(torch.randint(0, n_big, (1024,), generator=gen), n_big)
    small = Zones.from_labels(torch.randint(0, 8, (n_small,), generator=gen), num_zones=8)
    res = {"device": torch.cuda.get_device_name(0), "lib": _lib.lib_info()["sha256"],
           "series": [bench(n_big, 100, big, dev, 200 // q, 8 // q),
                      bench(n_small, 48, small, dev, 4000 // q, 200 // q)]}
    # what the large figure depends on: full 64-step tiles and line-aligned rows (T = 128), and
    # zones of consecutive rows in place of scattered ones
    blocks = Zones.from_labels(torch.arange(n_big) // (n_big // 64), num_zones=64)
    res["sensitivity"] = []
    for name, zones, T in (("random", big, 128), ("random", big, 64), ("blocks", blocks, 100), ("blocks", blocks, 128)):
        r = bench(n_big, T, zones, dev, 100 // q, 1)
        res["sensitivity"].append({"zones": name, **{k: r[k] for k in ("shape", "listed_rows", "kernel_us", "torch_us",
                                                                        "kernel_bytes_per_s",
                                                                        "fraction_of_hbm_achievable_6p3TBs")}})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
