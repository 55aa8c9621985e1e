"""The raster kernels: the locate step on its own, and sample / frames against the same products
composed from torch ops on the same device.

    python tools/raster_bench.py [--out profiles/raster/bench.json] [--quick]

Sizes: the finest scale of zenodo4 (10,368 faces) onto 1,024 x 1,024 pixels, and the finest scale
of hbm1m (1,002,528 faces) onto 4,096 x 4,096, each grid covering the mesh's bounding box.
  * locate: 9 handles created one after the other; of each, the host seconds of the checks, face
    records and bucket grid (``host_build_seconds``) and the device time of k_raster_locate between
    two events on its stream (``locate_us``) -- reported separately, medians with min and max.
    There is no torch composition to compare with.  Before timing, every pixel's face is checked to
    contain the pixel centre (the edge functions restated in torch float64 on the device).
  * sample: 9 float32 layers against ``torch.where(pr >= 0, layers[:, pr.clamp(min=0)], nodata)``
    (pr converted to int64 once, outside the timed windows).
  * frames: a 16-step window (steps 16..31) of a T = 48 rollout against
    ``torch.where(pr >= 0, pred[pr.clamp(min=0), 0, 16:32].permute(2, 0, 1), nodata).contiguous()``.
The two sides' outputs are compared bit for bit before timing.  Timing: warm-up, then 9 repeats in
which the two sides alternate, each repeat a window of calls under a host clock that ends in a
device synchronise; medians.  Algorithmic bytes per pixel -- sample reads 4 + 4 L and writes 4 L,
frames reads 4 + 4 t_count and writes 4 t_count -- over the median time, also as a fraction of the
~6.3 TB/s achievable HBM rate.  Needs a GPU; there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mswe-gnn_amd"))

from mswegnn import _lib  # noqa: E402
from mswegnn.mesh import mesh_config, multiscale_geometry  # noqa: E402
from mswegnn.raster import RasterGrid, Rasterizer  # noqa: E402

HBM_ACHIEVABLE = 6.3e12
REPEATS = 9
LAYERS, T, T_BEGIN, T_COUNT = 9, 48, 16, 16


def window(fn, calls):
    """Seconds per call of ``calls`` calls under a host clock that ends in a device synchronise."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def alternate(kernel, composed, calls_kernel, calls_torch):
    for _ in range(3):
        kernel()
        composed()
    tk, tt = [], []
    for _ in range(REPEATS):
        tk.append(window(kernel, calls_kernel))
        tt.append(window(composed, calls_torch))
    return (statistics.median(tk), min(tk), max(tk)), (statistics.median(tt), min(tt), max(tt))


def record(tk, tt, pixels, bytes_per_pixel, calls_kernel, calls_torch):
    nbytes = pixels * bytes_per_pixel
    return {"bytes_per_pixel": bytes_per_pixel, "algorithmic_bytes": nbytes, "repeats": REPEATS,
            "kernel_us": tk[0] * 1e6, "kernel_us_min_max": [tk[1] * 1e6, tk[2] * 1e6], "kernel_calls_per_window": calls_kernel,
            "torch_us": tt[0] * 1e6, "torch_us_min_max": [tt[1] * 1e6, tt[2] * 1e6], "torch_calls_per_window": calls_torch,
            "speedup_vs_torch": tt[0] / tk[0], "kernel_beats_torch": bool(tk[0] < tt[0]),
            "kernel_bytes_per_s": nbytes / tk[0], "fraction_of_hbm_achievable_6p3TBs": nbytes / tk[0] / HBM_ACHIEVABLE}


def contained(xy, faces, grid, pr):
    """Every pixel with a face lies in it: the header's edge functions in torch float64."""
    dev = pr.device
    x, y = torch.from_numpy(xy[:, 0].copy()).to(dev), torch.from_numpy(xy[:, 1].copy()).to(dev)
    fn = torch.from_numpy(faces).to(dev).long()
    px = (grid.x0 + torch.arange(grid.width, device=dev, dtype=torch.float64) * grid.dx)[None, :].expand(grid.shape)
    py = (grid.y0 + torch.arange(grid.height, device=dev, dtype=torch.float64) * grid.dy)[:, None].expand(grid.shape)
    hit = pr >= 0
    f = pr[hit].long()
    px, py = px[hit], py[hit]
    a, b, c = fn[f, 0], fn[f, 1], fn[f, 2]
    area2 = (x[b] - x[a]) * (y[c] - y[a]) - (y[b] - y[a]) * (x[c] - x[a])
    ok = torch.ones_like(f, dtype=torch.bool)
    for u, v in ((a, b), (b, c), (c, a)):
        p, q = torch.minimum(u, v), torch.maximum(u, v)
        e = (x[q] - x[p]) * (py - y[p]) - (y[q] - y[p]) * (px - x[p])
        e = torch.where(u < v, e, -e)
        ok &= torch.where(area2 > 0, e >= 0, e <= 0)
    return bool(ok.all()), int(hit.sum())


def bench(name, side, dev, calls):
    cfg = mesh_config(name)
    t0 = time.perf_counter()
    xy, faces = multiscale_geometry(cfg["n_coarse"], cfg["num_scales"], 0)[0]
    geometry_seconds = time.perf_counter() - t0
    (xlo, ylo), (xhi, yhi) = xy.min(0), xy.max(0)
    grid = RasterGrid(xlo, yhi, (xhi - xlo) / (side - 1), -(yhi - ylo) / (side - 1), side, side)
    P, n = side * side, len(faces)

    host, loc, r = [], [], None
    for _ in range(REPEATS):
        if r is not None:
            r.close()
        r = Rasterizer(xy, faces, grid, device=dev)
        s = r.stats()
        host.append(s["host_build_seconds"])
        loc.append(s["locate_us"])
    pr = r.pixel_rows
    inside, hits = contained(xy, faces, grid, pr)
    g, per, it = r.launch()
    locate = {"launch": {"grid": g, "pixels_per_wg": per, "iters": it}, "repeats": REPEATS,
              "host_build_seconds": statistics.median(host), "host_build_seconds_min_max": [min(host), max(host)],
              "locate_us": statistics.median(loc), "locate_us_min_max": [min(loc), max(loc)],
              "pixels_per_us": P / statistics.median(loc), "pixels_with_a_face": hits,
              "every_found_face_contains_its_pixel": inside,
              **{k: s[k] for k in ("buckets", "buckets_x", "buckets_y", "list_entries", "longest_list", "device_bytes")}}

    gen = torch.Generator(device=dev).manual_seed(0)
    layers = torch.rand(LAYERS, n, device=dev, generator=gen)
    pred = torch.rand(n + 1, 2, T, device=dev, generator=gen)
    prl = pr.long().clamp(min=0)
    hit = pr >= 0
    nodata = torch.full((), float("nan"), device=dev)

    def sample_torch():
        return torch.where(hit, layers[:, prl], nodata)

    def frames_torch():
        return torch.where(hit, pred[prl, 0, T_BEGIN:T_BEGIN + T_COUNT].permute(2, 0, 1), nodata).contiguous()

    same_s = bool(torch.equal(r.sample(layers).view(torch.int32), sample_torch().view(torch.int32)))
    same_f = bool(torch.equal(r.frames(pred, 0, T_BEGIN, T_COUNT).view(torch.int32), frames_torch().view(torch.int32)))
    tk, tt = alternate(lambda: r.sample(layers), sample_torch, calls[0], calls[1])
    sample = {"layers": LAYERS, "equals_torch_bitwise": same_s, **record(tk, tt, P, 4 + 8 * LAYERS, calls[0], calls[1])}
    tk, tt = alternate(lambda: r.frames(pred, 0, T_BEGIN, T_COUNT), frames_torch, calls[0], calls[1])
    frames = {"T": T, "window": [T_BEGIN, T_COUNT], "equals_torch_bitwise": same_f,
              **record(tk, tt, P, 4 + 8 * T_COUNT, calls[0], calls[1])}
    r.close()
    return {"mesh": name, "faces": n, "grid": [side, side], "pixels": P, "geometry_seconds_python": geometry_seconds,
            "locate": locate, "sample": sample, "frames": frames}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raster", "bench.json"))
    ap.add_argument("--quick", action="store_true", help="fewer calls per timing window")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("raster_bench needs a GPU")
    dev = torch.device("cuda:0")
    q = 4 if a.quick else 1
    res = {"device": torch.cuda.get_device_name(0), "lib": _lib.lib_info()["sha256"],
           "note": "kernel sides include the wrapper's output allocation (torch.empty), as the torch sides do",
           "sizes": [bench("zenodo4", 1024, dev, (400 // q, 100 // q)), bench("hbm1m", 4096, dev, (40 // q, 12 // q))]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
