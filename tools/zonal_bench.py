"""The zonal kernels: building the cell pixel lists, and reduce / frames_to_rows against the same
statistics composed from torch ops on the same device.

    python tools/zonal_bench.py [--out profiles/zonal/bench.json] [--quick] [--mappings]

Sizes: zenodo4 (finest scale 10,368 faces, coarsest 162) under 1,024 x 1,024 pixels and hbm1m
(finest 1,002,528 faces, coarsest 62,658) under 4,096 x 4,096, each grid covering the mesh's
bounding box -- lists of about 17 pixels (a lane per face), 101 and 268 (the wave per face) and
6,473 (few faces, long lists).
  * create: 9 handles made one after the other from one raster handle; ``build_us`` (host clock
    around the kernels, the copies and the host prefix sum), median with min and max.
  * reduce: 9 float32 layers, all four outputs, against float64 ``index_add_`` for the sums and
    counts plus ``scatter_reduce`` with amin / amax over ``pixel_rows`` (indices converted to int64
    once, outside the timed windows).  The counts and extremes are compared bit for bit before
    timing, the means within 1 ulp (the composition's atomic sums have no fixed order).
  * frames_to_rows: a 16-frame window into steps 16..31 of a T = 48 array, against the composed
    mean written through an index.
Timing: every shape warmed, then 9 repeats in which the two sides alternate, each repeat a window
of calls between two device events (windows of about 0.2 s; 3 repeats where one call of the
composition alone takes over half a second); medians.  Progress goes to stderr.  Algorithmic bytes -- reduce reads 4 P (L + 1) (the
layers and the lists) and writes 16 L faces, frames_to_rows reads 4 P (t_count + 1) and writes
4 t_count faces -- over the median time, also as a fraction of the ~6.3 TB/s achievable HBM rate.
``--mappings`` repeats the reduce timings in child processes under the build variants
``zonallane`` and ``zonalwave`` (one mapping for every list; built first if their libraries are
missing).  Needs a GPU; there is no fallback.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mswe-gnn_amd"))

from mswegnn import _lib  # noqa: E402
from mswegnn.mesh import mesh_config, multiscale_geometry  # noqa: E402
from mswegnn.raster import RasterGrid, Rasterizer  # noqa: E402

HBM_ACHIEVABLE = 6.3e12
REPEATS = 9
LAYERS, T, T_BEGIN, T_COUNT = 9, 48, 16, 16
SIZES = (("zenodo4", 1024, 0), ("zenodo4", 1024, -1), ("hbm1m", 4096, 0), ("hbm1m", 4096, -1))


def log(msg):
    print(msg, file=sys.stderr, flush=True)


def window(fn, calls):
    """Seconds per call of ``calls`` calls between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / calls


def plan(fn, most):
    """One warm call, timed; then (calls per window, repeats): windows of about 0.2 s, at most
    ``most`` calls, and 3 repeats instead of 9 where one call alone takes over half a second (the
    composition's atomics on a scale of a few faces)."""
    fn()
    t = window(fn, 1)
    if t < 0.05:
        fn()
    return max(1, min(most, int(0.2 / t))), (REPEATS if t < 0.5 else 3)


def alternate(kernel, composed, most_kernel, most_torch, what):
    ck, rk = plan(kernel, most_kernel)
    ct, rt = plan(composed, most_torch) if composed else (0, 0)
    log(f"  {what}: {ck} kernel calls x {rk} windows, {ct} torch calls x {rt}")
    tk, tt = [], []
    for i in range(rk):
        tk.append(window(kernel, ck))
        if i < rt:
            tt.append(window(composed, ct))
    stat = lambda t, c: {"median": statistics.median(t), "min": min(t), "max": max(t), "calls": c, "repeats": len(t)}  # noqa: E731
    return stat(tk, ck), (stat(tt, ct) if composed else None)


def record(tk, tt, nbytes):
    out = {"algorithmic_bytes": nbytes, "repeats": tk["repeats"], "kernel_us": tk["median"] * 1e6,
           "kernel_us_min_max": [tk["min"] * 1e6, tk["max"] * 1e6], "kernel_calls_per_window": tk["calls"],
           "kernel_bytes_per_s": nbytes / tk["median"],
           "fraction_of_hbm_achievable_6p3TBs": nbytes / tk["median"] / HBM_ACHIEVABLE}
    if tt:
        out.update({"torch_us": tt["median"] * 1e6, "torch_us_min_max": [tt["min"] * 1e6, tt["max"] * 1e6],
                    "torch_calls_per_window": tt["calls"], "torch_repeats": tt["repeats"],
                    "speedup_vs_torch": tt["median"] / tk["median"], "kernel_beats_torch": bool(tk["median"] < tt["median"])})
    return out


def ulps(a, b):
    return int((a.view(torch.int32).long() - b.view(torch.int32).long()).abs().max())


_GEOMETRY = {}


def bench(name, side, scale, dev, calls, compose=True):
    if name not in _GEOMETRY:
        cfg = mesh_config(name)
        _GEOMETRY[name] = multiscale_geometry(cfg["n_coarse"], cfg["num_scales"], 0)
    xy, faces = _GEOMETRY[name][scale]
    (xlo, ylo), (xhi, yhi) = xy.min(0), xy.max(0)
    grid = RasterGrid(xlo, yhi, (xhi - xlo) / (side - 1), -(yhi - ylo) / (side - 1), side, side)
    P, n = side * side, len(faces)
    log(f"{name}[{scale}]: {n} faces under {side} x {side}")
    r = Rasterizer(xy, faces, grid, device=dev)
    log("  located")
    build, cp = [], None
    for _ in range(REPEATS):
        if cp is not None:
            cp.close()
        cp = r.cells()
        build.append(cp.stats()["build_us"])
    s = cp.stats()
    log(f"  lists built: {statistics.median(build):.0f} us, longest {s['longest_list']}")
    g, per, it = cp.launch()
    res = {"mesh": name, "scale": scale, "faces": n, "grid": [side, side], "pixels": P,
           "mean_list": s["listed_pixels"] / max(n - s["empty_faces"], 1),
           "launch": {"grid": g, "faces_per_wg": per, "iters": it}}
    create = {"repeats": REPEATS, "build_us": statistics.median(build), "build_us_min_max": [min(build), max(build)],
              "pixels_per_us": P / statistics.median(build),
              **{k: s[k] for k in ("listed_pixels", "longest_list", "empty_faces", "device_bytes")}}

    gen = torch.Generator(device=dev).manual_seed(0)
    layers = torch.rand(LAYERS, side, side, device=dev, generator=gen)
    stack = torch.rand(T_COUNT, side, side, device=dev, generator=gen)
    pred = torch.zeros(n + 1, 2, T, device=dev)
    outs = {"mean": torch.empty(LAYERS, n, device=dev), "count": torch.empty(LAYERS, n, dtype=torch.int32, device=dev),
            "min": torch.empty(LAYERS, n, device=dev), "max": torch.empty(LAYERS, n, device=dev)}

    def reduce_kernel():
        return cp.reduce(layers, out=outs)

    def frames_kernel():
        return cp.frames_to_rows(stack, pred, 0, T_BEGIN)

    nb_reduce = 4 * P * (LAYERS + 1) + 16 * LAYERS * n
    nb_frames = 4 * P * (T_COUNT + 1) + 4 * T_COUNT * n
    if not compose:
        tk, _ = alternate(reduce_kernel, None, calls[0], 0, "reduce")
        res["reduce"] = record(tk, None, nb_reduce)
        cp.close()
        r.close()
        return res

    pr = r.pixel_rows.reshape(-1)
    hit = pr >= 0
    idx = pr[hit].long()
    idx_l = idx.expand(LAYERS, -1)
    centre = cp.centre_pixel.long().clamp(min=0)

    def stats_torch(x):
        """mean (float64 index_add_), count, min, max of x [L, H, W]; empty cells take the centre pixel."""
        v = x.reshape(x.shape[0], -1)
        vals = v[:, hit]
        total = torch.zeros(x.shape[0], n, dtype=torch.float64, device=dev).index_add_(1, idx, vals.double())
        count = torch.zeros(n, dtype=torch.float64, device=dev).index_add_(0, idx, torch.ones_like(idx, dtype=torch.float64))
        fill = v[:, centre]
        return torch.where(count > 0, (total / count).float(), fill), count, vals, fill

    def reduce_torch():
        mean, count, vals, fill = stats_torch(layers)
        lo = torch.full((LAYERS, n), float("inf"), device=dev).scatter_reduce(1, idx_l, vals, "amin")
        hi = torch.full((LAYERS, n), float("-inf"), device=dev).scatter_reduce(1, idx_l, vals, "amax")
        return mean, count, torch.where(count > 0, lo, fill), torch.where(count > 0, hi, fill)

    def frames_torch():
        pred[:n, 0, T_BEGIN:T_BEGIN + T_COUNT] = stats_torch(stack)[0].t()
        return pred

    log("  composing once for the checks")
    got = reduce_kernel()
    mean, count, lo, hi = reduce_torch()
    checks = {"count_equal": bool(torch.equal(got["count"][0].double(), count)),
              "min_max_equal_bitwise": bool(torch.equal(got["min"].view(torch.int32), lo.view(torch.int32))
                                            and torch.equal(got["max"].view(torch.int32), hi.view(torch.int32))),
              "mean_worst_ulp": ulps(got["mean"], mean)}
    want = frames_torch().clone()
    pred.zero_()
    checks["frames_worst_ulp"] = ulps(frames_kernel(), want)
    log(f"  checks: {checks}")
    tk, tt = alternate(reduce_kernel, reduce_torch, calls[0], calls[1], "reduce")
    res["create"] = create
    res["checks"] = checks
    res["reduce"] = {"layers": LAYERS, **record(tk, tt, nb_reduce)}
    tk, tt = alternate(frames_kernel, frames_torch, calls[0], calls[1], "frames_to_rows")
    res["frames_to_rows"] = {"T": T, "window": [T_BEGIN, T_COUNT], **record(tk, tt, nb_frames)}
    cp.close()
    r.close()
    return res


def calls_for(side, quick):
    """The most calls per window, (kernel, torch)."""
    q = 4 if quick else 1
    return (200 // q, 40 // q) if side <= 1024 else (20 // q, 8 // q)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zonal", "bench.json"))
    ap.add_argument("--quick", action="store_true", help="fewer calls per timing window")
    ap.add_argument("--mappings", action="store_true", help="also time reduce under the zonallane / zonalwave builds")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("zonal_bench needs a GPU")
    dev = torch.device("cuda:0")
    if a.child:   # reduce alone, under the library MSW_LIB_VARIANT names
        print(json.dumps([bench(m, side, sc, dev, calls_for(side, a.quick), compose=False) for m, side, sc in SIZES]))
        return
    res = {"device": torch.cuda.get_device_name(0), "lib": _lib.lib_info()["sha256"],
           "note": "kernel sides include the wrapper's checks; outputs are allocated once, outside the windows",
           "sizes": []}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    for m, side, sc in SIZES:
        res["sizes"].append(bench(m, side, sc, dev, calls_for(side, a.quick)))
        save()
    if a.mappings:
        import build_engine
        res["mappings"] = {"chosen": {f"{s['mesh']}[{s['scale']}]": s["reduce"]["kernel_us"] for s in res["sizes"]}}
        for variant in ("zonallane", "zonalwave"):
            if not build_engine.library_matches_sources(variant):
                build_engine.build(verbose=False, variant=variant)
            log(f"mapping {variant}")
            env = dict(os.environ, MSW_LIB_VARIANT=variant)
            cmd = [sys.executable, os.path.abspath(__file__), "--child"] + (["--quick"] if a.quick else [])
            out = subprocess.run(cmd, env=env, check=True, stdout=subprocess.PIPE, text=True).stdout
            sizes = json.loads(out.strip().splitlines()[-1])
            res["mappings"][variant] = {f"{s['mesh']}[{s['scale']}]": s["reduce"]["kernel_us"] for s in sizes}
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
