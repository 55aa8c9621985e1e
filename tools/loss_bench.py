"""The fused training loss (csrc/loss.hip) against the torch composition of the same loss.

    python tools/loss_bench.py [--out profiles/loss/bench.json] [--quick]

Forward + backward of ``mswegnn.loss.loss_function`` (the HIP kernels) and of
``mswegnn.loss.torch_loss_function`` (the reference's ops in torch) on the same device tensors,
RMSE with velocity_scaler 7 (config.yaml), on seeded synthetic predictions of
  [13,774, 2]      the zenodo4 mesh (config 2: 10,369 finest rows of 13,774)
  [1,382,400, 2]   config 5's size (1,048,576 finest rows)
as one Data with node_ptr, variants: mask on / off x with / without the conservation term
(0.5).  About 40 % of the rows are dry in prediction and target, as on the flood fixtures.  Timed
with device events, 200 calls per window after warm-up, median of 5 windows, the two alternating;
the two losses and gradients are compared before timing.  The masked composition reads the device
inside every call (its boolean-mask index), so its figure includes that host round trip -- that
is what a training step pays.  Bytes the fused call must move: 16 per range row forward (pred,
real) + 24 backward (pred, real, the gradient) + 8 per other row (zero gradient), with the
conservation term 12 more per range row (area twice, input depth).  Needs a GPU; no fallback.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mswe-gnn_amd"))

from mswegnn import _lib  # noqa: E402
from mswegnn.loss import LOSS_CALLS, launch, loss_function, torch_loss_function  # noqa: E402
from mswegnn.mesh import Graph  # noqa: E402

HBM_ACHIEVABLE = 6.3e12
SIZES = (("zenodo4", 13774, 10369), ("config5", 1382400, 1048576))


def synthetic(n, fine, dev, seed=0):
    gen = torch.Generator(device=dev).manual_seed(seed)
    real = torch.rand(n, 2, device=dev, generator=gen) * 2
    preds = real + 0.1 * torch.randn(n, 2, device=dev, generator=gen)
    dry = torch.rand(n, device=dev, generator=gen) < 0.4
    real[dry], preds[dry] = 0.0, 0.0
    x = torch.rand(n, 8, device=dev, generator=gen)
    data = Graph(x=x, node_ptr=torch.tensor([0, fine, n], device=dev),
                 area=torch.rand(n, device=dev, generator=gen) * 50 + 10,
                 node_BC=torch.tensor([fine - 1], device=dev), edge_BC_length=torch.tensor([62.5], device=dev),
                 temporal_res=torch.tensor(120, device=dev))
    return preds.requires_grad_(True), real, data, torch.tensor([2.5], device=dev)


def time_pair(fns, iters, repeats=5):
    """Median seconds per call of each function: windows of `iters` calls, the functions alternating."""
    per = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            per[k].append(a.elapsed_time(b) * 1e-3 / iters)
    return [(statistics.median(p), min(p), max(p)) for p in per]


def bench(name, n, fine, dev, iters):
    preds, real, data, BC = synthetic(n, fine, dev)
    out = {"name": name, "shape": [n, 2], "fine_rows": fine,
           "launch": dict(zip(("grid", "rows_per_wg", "iters"), launch(fine))), "variants": []}
    for mask in (True, False):
        for c in (0.0, 0.5):
            kw = dict(type_loss="RMSE", only_where_water=mask, conservation=c, velocity_scaler=7)

            def run(fn):
                preds.grad = None
                loss = fn(preds, real, data, BC, **kw)
                loss.backward()
                return loss

            def fused():
                return run(loss_function)

            def composed():
                return run(torch_loss_function)
            calls = LOSS_CALLS[0]
            lf = float(fused())
            gf = preds.grad.clone()
            assert LOSS_CALLS[0] == calls + 1, "the HIP loss did not run"
            lt = float(composed())
            gt = preds.grad.clone()
            for _ in range(10):
                fused()
                composed()
            torch.cuda.synchronize()
            tf, tt = time_pair((fused, composed), iters)
            nbytes = 40 * fine + 8 * (n - fine) + (12 * fine if c else 0)
            out["variants"].append({
                "only_where_water": mask, "conservation": c, "loss_fused": lf, "loss_torch": lt,
                "loss_rel_diff": abs(lf - lt) / abs(lt),
                "grad_rel_diff": float((gf - gt).abs().max() / gt.abs().max()),
                "fused_s": tf[0], "fused_s_min_max": tf[1:], "torch_s": tt[0], "torch_s_min_max": tt[1:],
                "calls_per_window": iters, "speedup_vs_torch": tt[0] / tf[0], "bytes": nbytes,
                "fused_bytes_per_s": nbytes / tf[0],
                "fraction_of_hbm_achievable_6p3TBs": nbytes / tf[0] / HBM_ACHIEVABLE})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss", "bench.json"))
    ap.add_argument("--quick", action="store_true", help="fewer calls per timing window")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_bench needs a GPU")
    dev = torch.device("cuda:0")
    iters = 50 if a.quick else 200
    res = {"device": torch.cuda.get_device_name(0), "lib": _lib.lib_info()["sha256"],
           "what": "forward + backward of one loss call, seconds per call (median of 5 windows)",
           "sizes": [bench(name, n, fine, dev, iters) for name, n, fine in SIZES]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
