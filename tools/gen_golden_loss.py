"""Golden training losses (tests/golden/fx_loss.npz), made by the REFERENCE's own loss_function
and torch autograd (test infrastructure only; runs where the reference tree exists):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_loss.py [reference root]

Layouts (inputs stored once per layout LAYOUT/...: preds, real, x_h = data.x[:, -2], area, node_bc,
bc, edge_bc_length, temporal_res, ranges, num_graphs):
  data    the tiny multi-scale mesh as one Data (node_ptr [S + 1])
  batch   the tiny and the small mesh as a two-graph Batch through the reference's
          adapt_batch_training (node_ptr [G, S + 1], num_graphs = 2)
  single  a single-scale mesh without node_ptr
with the meshes' raw cell areas, finest BC edge length and hydrograph, as
oracle/gen_golden_metrics.py builds them.  preds / real: full-precision fp32 values, about 40 % of
the rows dry in both (outside mask_on_water), some rows differing in one variable only.
Cases LAYOUT/TYPE_mMASK_vVS_cC: loss_function(preds, real, data, BC, type_loss=TYPE,
only_where_water=MASK, conservation=C, velocity_scaler=VS) for RMSE / MAE x mask 0 / 1 x
velocity_scaler 1 / 7 x conservation 0 / 0.5 -> .../loss and .../grad, the autograd gradient with
respect to preds.  The conservation cases of RMSE use x_h (cons > 0), those of MAE x_h_neg
(cons < 0); .../cons holds conservation_loss itself.  batch/alias: data.x rebuilt from preds as
training_step does (use_prediction), so that data.x[:, -2] is preds[:, 0] through autograd.
No reference source is copied; oracle/ is read (its import stubs), nothing there is modified.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.path[:0] = [os.path.join(ROOT, "oracle", "refstubs"), REF]
sys.dont_write_bytecode = True

from training.loss import conservation_loss, loss_function  # noqa: E402
from training.train import adapt_batch_training  # noqa: E402
from utils.dataset import use_prediction  # noqa: E402
from torch_geometric.data import Batch, Data  # noqa: E402  (oracle/refstubs attribute bags)

TYPES, MASKS, SCALERS, CONS = ("RMSE", "MAE"), (0, 1), (1, 7), (0.0, 0.5)
BC_STEP = 2


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def case_name(tl, mask, vs, c):
    return f"{tl}_m{mask}_v{vs}_c{c}"


def states(n, seed):
    """preds, real [n, 2] and the two input depths (cons > 0 / cons < 0)."""
    gen = torch.Generator().manual_seed(seed)
    real = torch.rand(n, 2, generator=gen) * torch.tensor([2.0, 3.0]) - torch.tensor([0.0, 1.5])
    preds = real + 0.1 * torch.randn(n, 2, generator=gen)
    kind = torch.arange(n) % 10
    dry = kind < 4
    real[dry], preds[dry] = 0.0, 0.0
    preds[kind == 4, 1] = real[kind == 4, 1]   # only h differs
    preds[kind == 5, 0] = real[kind == 5, 0]   # only v differs
    preds[:, 0] = preds[:, 0].clamp_min(0)
    # the volume grows by more than the inflow (cons > 0; such a rise needs depths below the bed)
    x_h = preds[:, 0] - 1.5 - torch.rand(n, generator=gen)
    x_h_neg = preds[:, 0] + 0.25 * torch.rand(n, generator=gen)                # it shrinks: cons < 0
    return preds.contiguous(), real.contiguous(), x_h, x_h_neg


def with_depth(data, x_h):
    d = data.clone()
    d.x = d.x.clone()
    d.x[:, -2] = x_h
    return d


def main():
    sys.path.insert(0, os.path.join(ROOT, "mswe-gnn_amd"))
    from mswegnn.mesh import make_multiscale_mesh, make_single_scale_mesh, mesh_config

    def member(name):
        g = make_multiscale_mesh(**mesh_config(name), T=4)
        g.edge_BC_length = g.edge_BC_length[:1].clone()   # the finest scale's
        g.node_BC = g.node_BC.long()
        return Data(**g.__dict__)

    tiny, small = member("tiny"), member("small")
    s = make_single_scale_mesh(n_coarse=3, refinements=3, T=4)
    s.node_BC = s.node_BC.long()
    layouts = {"data": tiny.clone(), "batch": adapt_batch_training(Batch.from_data_list([tiny, small])),
               "single": Data(**s.__dict__)}
    out = {"cpu": np.array(cpu_model()), "bc_step": np.array(BC_STEP)}
    names = []
    for li, (lname, data) in enumerate(layouts.items()):
        n = data.x.shape[0]
        preds0, real, x_h, x_h_neg = states(n, 100 + li)
        BC = data.BC[:, -2:, BC_STEP].mean(1)   # training_step's argument (train.py:138)
        batch = isinstance(data, Batch)
        if "node_ptr" in data.keys():
            ptr = data.node_ptr.reshape(-1, data.node_ptr.shape[-1])
            ranges = [[int(r[0]), int(r[1])] for r in ptr]
        else:
            ranges = [[0, n]]
        out.update({f"{lname}/preds": preds0.numpy(), f"{lname}/real": real.numpy(), f"{lname}/x_h": x_h.numpy(),
                    f"{lname}/x_h_neg": x_h_neg.numpy(), f"{lname}/area": data.area.numpy(),
                    f"{lname}/node_bc": data.node_BC.numpy(), f"{lname}/bc": BC.numpy(),
                    f"{lname}/edge_bc_length": np.broadcast_to(data.edge_BC_length.numpy(), BC.shape).copy(),
                    f"{lname}/temporal_res": np.asarray(data.temporal_res), f"{lname}/ranges": np.array(ranges),
                    f"{lname}/num_graphs": np.array(data.num_graphs if batch else 1),
                    f"{lname}/is_batch": np.array(batch), f"{lname}/has_node_ptr": np.array("node_ptr" in data.keys())})
        for tl in TYPES:
            for mask in MASKS:
                for vs in SCALERS:
                    for c in CONS:
                        d = with_depth(data, x_h if tl == "RMSE" else x_h_neg)
                        preds = preds0.clone().requires_grad_(True)
                        loss = loss_function(preds, real, d, BC, type_loss=tl, only_where_water=bool(mask),
                                             conservation=c, velocity_scaler=vs)
                        loss.backward()
                        key = f"{lname}/{case_name(tl, mask, vs, c)}"
                        names.append(key)
                        out[key + "/loss"] = loss.detach().numpy()
                        out[key + "/grad"] = preds.grad.numpy()
                        if c:
                            with torch.no_grad():
                                out[key + "/cons"] = conservation_loss(preds[:, 0::2], d.x[:, -2::2], d, BC).numpy()
        if lname == "batch":   # data.x[:, -2] IS preds[:, 0], through another autograd path
            preds = preds0.clone().requires_grad_(True)
            d = data.clone()
            d.x = use_prediction(data.x.clone(), preds, 3)
            loss = loss_function(preds, real, d, BC, type_loss="RMSE", only_where_water=True, conservation=0.5,
                                 velocity_scaler=7)
            loss.backward()
            names.append("batch/alias")
            out["batch/alias/loss"], out["batch/alias/grad"] = loss.detach().numpy(), preds.grad.numpy()
    out["cases"] = np.array(names)
    path = os.path.join(ROOT, "tests", "golden", "fx_loss.npz")
    np.savez_compressed(path, **out)
    signs = {k: float(v) for k, v in out.items() if k.endswith("/cons")}
    assert any(v > 0 for v in signs.values()) and any(v < 0 for v in signs.values()), signs
    # the fixture carries its own record (cpu, cases): tests/golden/manifest.json is not touched
    print(len(names), "cases;", os.path.getsize(path), "bytes; cons", signs)


if __name__ == "__main__":
    main()
