"""Generate the layout fixtures by running the REFERENCE itself (test infrastructure only).

Runs only in the build container, where /root/reference exists:

    PYTHONDONTWRITEBYTECODE=1 python oracle/gen_golden_layout.py

Like oracle/gen_golden.py: oracle/refstubs and /root/reference on sys.path, the reference's own
MSGNN / GNN modules (models/gnn.py) built with the constructor arguments of a layout case
(tests/layout_cases.py model_kwargs), its seeded init made sensitive by layout_cases.sensitize,
one forward and the reference's own ``training.train.rollout_test`` over p + 3 steps on the
case's graph (layout_cases.make_graph).  Writes tests/golden/fx_layout_<case>.npz: the graph
digest, the exported weights (``w__<state-dict key>``), the one-step output, the rollout and the
generating CPU model; no reference source is copied.  The oracle restatement is checked against
the same outputs here (bit for bit); tests/test_layout.py repeats that check without the
reference.
"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
# the stand-ins and the reference first: its models/ is a namespace package, the drop-in's
# regular ``models`` package would win from any position on sys.path
sys.path[:0] = [os.path.join(ROOT, "oracle", "refstubs"), REF]
sys.dont_write_bytecode = True

from models.gnn import MSGNN, GNN  # noqa: E402  (the reference's modules)
from training.train import rollout_test  # noqa: E402
import models.gnn as _refgnn  # noqa: E402
assert _refgnn.__file__.startswith(REF), _refgnn.__file__
sys.path += [os.path.join(ROOT, "mswe-gnn_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import layout_cases as lc  # noqa: E402
import msgnn_torch as orc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
torch.set_num_threads(8)


def graph_digest(g):
    h = hashlib.sha256()
    for k in ("x", "edge_index", "edge_attr", "edge_ptr", "node_ptr", "intra_mesh_edge_index",
              "intra_edge_ptr", "BC", "node_BC"):
        if k in g.keys():
            h.update(np.ascontiguousarray(getattr(g, k).numpy()).tobytes())
    return np.frombuffer(bytes.fromhex(h.hexdigest()), np.uint8)


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def main():
    for combo in lc.FIXTURES:
        case, kind, F = combo
        model = (GNN if kind == "gnn" else MSGNN)(**lc.model_kwargs(case, kind, F))
        P, amp = lc.sensitize(model.state_dict())
        model.load_state_dict(P, strict=True)
        model.eval()
        g, T, cfg = lc.make_graph(case, kind), lc.steps(case), lc.oracle_cfg(case, kind, F)
        with torch.no_grad():
            y = model(g)
            r = rollout_test(model, g)
        assert r.shape == (g.x.shape[0], 2, T)
        for what, ref, got in (("step", y, orc.forward(P, cfg, g)), ("rollout", r, orc.rollout(P, cfg, g, T))):
            d = (got - ref).abs().max().item()
            print(f"  oracle vs reference [{lc.combo_id(combo)} {what}]: max|diff| = {d:.3e}")
            assert d == 0.0, "oracle restatement is not bit-identical to the reference"
        name = lc.fixture_name(combo)
        # "cpu": the generating CPU model (these fixtures may come from another machine than
        # manifest.json's): bit-exact there, 1e-5 per step elsewhere
        arrays = dict(digest=graph_digest(g), y=y.numpy(), rollout=r.numpy(), amp=np.float32(amp),
                      cpu=np.array(cpu_model()))
        arrays.update({"w__" + k: v.numpy() for k, v in P.items()})
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(f"  wrote {name}.npz ({os.path.getsize(path) / 1e3:.0f} kB), max|rollout| {r.abs().max():.3f}")


if __name__ == "__main__":
    main()
