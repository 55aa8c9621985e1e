"""ORACLE / fixture generator (test infrastructure only): the REFERENCE's own MSGNN.forward and
rollout_test, with the shipped K4_F32 checkpoint, on irregular, renumbered meshes
(mswegnn.mesh.irregularize, order="canonical": moved and dropped (coarse, fine) pairs, deleted
finest faces, permuted ids -- what the reference's real meshes look like and the quadtree
generator never produces).

    PYTHONDONTWRITEBYTECODE=1 python oracle/gen_golden_irregular.py

Writes tests/golden/
* fx_irr_tiny_K4_F32_step          -- one MSGNN.forward (models/gnn.py:267-350), wet tiny mesh;
* fx_irr_small_K4_F32_rollout48    -- training/train.py:67-95 rollout_test, 48 steps from a dry
                                      start driven by the hydrograph (small mesh);
* fx_irr_small_K4_F32_wet_rollout8 -- the same for 8 steps from a wet start;
each with the digest of its input graph only (the tests rebuild the graph from the arguments in
the manifest's "fx_irr_spec" and check the digest), and checks the oracle restatement
(oracle/msgnn_torch.py) against all three bit for bit.  Adds its entries to the manifest and
regenerates nothing else.  Same import recipe as oracle/gen_golden.py (oracle/refstubs, the
reference from /root/reference); no reference source is copied.
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.dont_write_bytecode = True
import gen_golden as gg  # noqa: E402  (reference import, ref_msgnn, load_ckpt, graph_digest, save, check_oracle)

from training.train import rollout_test  # noqa: E402  (the reference's)
from mswegnn.mesh import irregularize, make_multiscale_mesh, mesh_config, wet_state  # noqa: E402
import msgnn_torch as orc  # noqa: E402

# name -> how the tests rebuild the input graph: make_multiscale_mesh(**mesh_config(mesh), T=T),
# wet_state(seed=wet) unless None, irregularize(seed=seed, order="canonical") at the default rates
SPEC = {
    "fx_irr_tiny_K4_F32_step": dict(mesh="tiny", T=48, wet=1, seed=0, steps=0),
    "fx_irr_small_K4_F32_rollout48": dict(mesh="small", T=48, wet=None, seed=2, steps=48),
    "fx_irr_small_K4_F32_wet_rollout8": dict(mesh="small", T=8, wet=4, seed=3, steps=8),
}


def build(spec):
    g = make_multiscale_mesh(**mesh_config(spec["mesh"]), T=spec["T"])
    if spec["wet"] is not None:
        g = wet_state(g, seed=spec["wet"])
    return irregularize(g, spec["seed"], order="canonical")[0]


def main():
    t0 = time.time()
    cfg = orc.msgnn_config(num_scales=4, hid_features=32, K=4)
    model = gg.ref_msgnn(cfg, gg.load_ckpt("K4_F32"))
    P = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for name, spec in SPEC.items():
        g = build(spec)
        digest = np.frombuffer(bytes.fromhex(gg.graph_digest(g)), np.uint8)
        with torch.no_grad():
            if spec["steps"]:
                r = rollout_test(model, g)
                assert r.shape[-1] == spec["steps"]
                gg.check_oracle(P, cfg, g, r, steps=spec["steps"], label=name)
                gg.save(name, rollout=r, digest=digest)
                print(f"  {name}: max h {r[:, 0].max():.3f}, wet cells at T: {(r[:, 0, -1] > 0).sum().item()} "
                      f"of {r.shape[0]}")
            else:
                y = model(g)
                gg.check_oracle(P, cfg, g, y, label=name)
                gg.save(name, y=y, digest=digest)
    path = os.path.join(ROOT, "tests", "golden", "manifest.json")
    with open(path) as f:
        full = json.load(f)
    full.update(gg.manifest)
    full["fx_irr_spec"] = SPEC
    with open(path, "w") as f:
        json.dump(full, f, indent=1)
    print(f"done in {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()
