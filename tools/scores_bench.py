"""The ensemble-scores kernel against the same scores composed from torch ops on the same device.

    python tools/scores_bench.py [--out profiles/ensemble/scores_bench.json] [--quick]

Seeded synthetic rollouts (tools/ensemble_bench.py's), thresholds 0.05 / 0.3; the truth is one more
run in the same array, so M + 1 runs are laid out:
  * 16 x 10,369 cells, T = 48: zenodo4 x 16 members, laid out as its batch is (3,405 coarse rows
    after every run's cells).  It sits in the caches: launch- and latency-bound, not a bandwidth;
  * [17 x 65,536, 2, 100]: the HBM-sized case of the sibling benches;
  * 64 x 10,369 cells, T = 48: the largest ensemble, where the M^2 rank counting dominates.
The kernel (msw_ensemble_scores_update, every output) runs against a composition over the
[M, n, T] view of the depths in float64: ``sort`` along the members for the pair sum, broadcasts
for the rest, ``index_add_`` for the table.  The composition materialises a sorted fp64 copy and
several [M, n, T] temporaries; it is what a user would write without the kernel.  The two sides
are compared before timing: the table exactly, the sums and cell_crps within 1e-9 relative (the
composition adds in torch's own order).
Timing: warm-up, then 9 repeats in which the two sides alternate, each repeat a window of calls
under a host clock that ends in a device synchronise; medians.  Algorithmic bytes: the kernel reads
(M + 1) n T 4; over the median time, also as a fraction of the ~6.3 TB/s achievable HBM rate.
Needs a GPU; there is no fallback.
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mswe-gnn_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ensemble_bench import THR, alternate, record, synthetic  # noqa: E402
from mswegnn import _lib  # noqa: E402
from mswegnn.ensemble import EnsembleScores, scores_launch  # noqa: E402


def bench(M, n, gap, T, dev, calls, note):
    N = (M + 1) * (n + gap)
    pred = synthetic(N, T, dev)
    ranges = [(m * (n + gap), m * (n + gap) + n) for m in range(M)]
    truth_row0 = M * (n + gap)
    lib = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    thr = (C.c_float * 2)(*THR)
    runs = pred.view(M + 1, n + gap, 2, T)[:, :n, 0, :]
    view, y32 = runs[:M], runs[M]                            # [M, n, T] and [n, T], strided: what a user holds

    es = EnsembleScores(ranges, T, THR, device=dev)
    o = _lib.MswEnsembleScoresOut(**{k: v.data_ptr() for k, v in es.arrays.items()})
    row0 = (C.c_int64 * M)(*[s for s, _ in ranges])
    p = C.c_void_p(pred.data_ptr())

    def kernel():
        rc = lib.msw_ensemble_scores_update(p, T, 0, T, row0, M, n, p, T, 0, truth_row0, thr, 2, T, 0, C.byref(o), st)
        if rc:
            _lib.check(rc)

    coef = (2.0 * torch.arange(M, device=dev, dtype=torch.float64) - M + 1)[:, None, None]
    col = torch.arange(T, device=dev)[None, :] * (M + 1)
    ones = torch.ones(n * T, dtype=torch.int64, device=dev)

    def composed():
        h, y = view.double(), y32.double()
        a = (h - y).abs().sum(0)
        b = (coef * torch.sort(h, dim=0).values).sum(0)
        S = h.sum(0)
        e = S - M * y
        v = M * (h * h).sum(0) - S * S
        sums = torch.stack([a.sum(0), b.sum(0), e.abs().sum(0), (e * e).sum(0), v.sum(0)], 1)
        table = torch.zeros(len(THR), 2, T * (M + 1), dtype=torch.int64, device=dev)
        for k, t in enumerate(THR):
            key = ((view > t).sum(0) + col).reshape(-1)
            table[k, 0].index_add_(0, key, ones)
            table[k, 1].index_add_(0, key, (y32 > t).reshape(-1).to(torch.int64))
        return sums, table.view(len(THR), 2, T, M + 1).permute(2, 0, 3, 1), (M * a - b).sum(1)

    kernel()
    sums, table, cell = composed()
    torch.cuda.synchronize()
    scale = sums.abs().amax(0).clamp_min(1e-300)
    same = {"reliability": bool(torch.equal(es.arrays["reliability"], table)),
            "sums_within_1e-9": bool(((es.arrays["sums"] - sums).abs() <= 1e-9 * scale).all()),
            "cell_crps_within_1e-9": bool(((es.arrays["cell_crps"] - cell).abs() <= 1e-9 * cell.abs().max()).all())}
    del sums, table, cell

    tk, tt = alternate(kernel, composed, calls[0], calls[1])     # later calls add onto cell_crps: the same work
    g, c, it = scores_launch(n, M, T)
    return {"shape": [N, 2, T], "members": M, "cells": n, "rows_between_runs": gap, "thresholds": list(THR), "note": note,
            "launch": {"grid": g, "cells_per_round": c, "rounds_per_tile": it}, "kernel_vs_torch": same,
            **record(tk, tt, (M + 1) * n * T * 4, calls[0], calls[1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble", "scores_bench.json"))
    ap.add_argument("--quick", action="store_true", help="fewer calls per timing window")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scores_bench needs a GPU")
    dev = torch.device("cuda:0")
    q = 4 if a.quick else 1
    res = {"device": torch.cuda.get_device_name(0), "lib": _lib.lib_info()["sha256"],
           "sizes": [bench(16, 10369, 3405, 48, dev, (400 // q, 40 // q), "cache-resident"),
                     bench(16, 65536, 0, 100, dev, (40 // q, 8 // q), "HBM-sized"),
                     bench(64, 10369, 3405, 48, dev, (40 // q, 8 // q), "largest ensemble")]}
    res["every_kernel_beats_torch"] = all(s["kernel_beats_torch"] for s in res["sizes"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
