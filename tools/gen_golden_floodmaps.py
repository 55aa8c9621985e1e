"""Golden flood maps (tests/golden/fx_floodmaps.npz), made by the REFERENCE's own functions
(test infrastructure only; runs where the reference tree exists):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_floodmaps.py [reference root]

Inputs: three committed rollouts, referred to by name (fx_small_K4_F32_rollout48,
fx_irr_small_K4_F32_rollout48, fx_irr_small_K4_F32_wet_rollout8; every row, every scale), the
thresholds 0, 0.05 and 0.3 m and the synthetic mesh's temporal_res.  Outputs, per rollout NAME:
  NAME/fat_THR_START    WD_to_FAT(h, temporal_res, THR, START) for START 0 and 2
                        (utils/miscellaneous.py:56-68)
  NAME/vel_max, NAME/froude_max   get_velocity(|q|, h).max(1), get_Froude(vel, h).max(1)
                        (utils/miscellaneous.py:44-54)
  NAME/h_max, NAME/q_max, NAME/t_h_max, NAME/t_q_max   h.max(1), |q|.max(1) and the first step
                        attaining each (numpy argmax: first occurrence)
  NAME/wet_steps_THR, NAME/first_wet_THR, NAME/last_wet_THR   steps with h > THR, first and last
                        of them (-1: never)
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

from utils.miscellaneous import WD_to_FAT, get_Froude, get_velocity  # noqa: E402

ROLLOUTS = ("fx_small_K4_F32_rollout48", "fx_irr_small_K4_F32_rollout48", "fx_irr_small_K4_F32_wet_rollout8")
THRESHOLDS = (0.0, 0.05, 0.3)
TIME_STARTS = (0, 2)


def main():
    g = os.path.join(ROOT, "tests", "golden")
    sys.path.insert(0, os.path.join(ROOT, "mswe-gnn_amd"))
    from mswegnn.mesh import make_multiscale_mesh, mesh_config
    temporal_res = make_multiscale_mesh(**mesh_config("small"), T=48).temporal_res
    out = {"rollouts": np.array(ROLLOUTS), "thresholds": np.array(THRESHOLDS, np.float32),
           "time_starts": np.array(TIME_STARTS), "temporal_res": np.asarray(temporal_res)}
    for name in ROLLOUTS:
        r = torch.from_numpy(np.load(os.path.join(g, name + ".npz"))["rollout"])
        h, q = r[:, 0, :].clone(), r[:, 1, :].abs()
        T = h.shape[1]
        vel = get_velocity(q.clone(), h.clone())
        out[f"{name}/vel_max"] = vel.max(1).values.numpy()
        out[f"{name}/froude_max"] = get_Froude(vel.clone(), h.clone()).max(1).values.numpy()
        out[f"{name}/h_max"] = h.max(1).values.numpy()
        out[f"{name}/q_max"] = q.max(1).values.numpy()
        out[f"{name}/t_h_max"] = np.argmax(h.numpy(), 1).astype(np.int32)
        out[f"{name}/t_q_max"] = np.argmax(q.numpy(), 1).astype(np.int32)
        for thr in THRESHOLDS:
            for ts in TIME_STARTS:
                out[f"{name}/fat_{thr}_{ts}"] = WD_to_FAT(h.clone(), temporal_res, thr, ts).numpy()
            wet = (h > thr).numpy()
            steps = np.arange(T, dtype=np.int32)
            out[f"{name}/wet_steps_{thr}"] = wet.sum(1).astype(np.int32)
            out[f"{name}/first_wet_{thr}"] = np.where(wet.any(1), np.argmax(wet, 1), -1).astype(np.int32)
            out[f"{name}/last_wet_{thr}"] = np.where(wet, steps, -1).max(1).astype(np.int32)
    np.savez_compressed(os.path.join(g, "fx_floodmaps.npz"), **out)
    print({k: (np.asarray(v).shape, np.asarray(v).dtype) for k, v in out.items()})
    print(os.path.getsize(os.path.join(g, "fx_floodmaps.npz")), "bytes")


if __name__ == "__main__":
    main()
