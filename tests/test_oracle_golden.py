"""The oracle (oracle/msgnn_torch.py) is pinned to outputs of the reference itself.

The fixtures were produced by running sdat2/mSWE-GNN's own MSGNN / GNN modules and
rollout_test on CPU (oracle/gen_golden.py, which also asserts oracle == reference bit for
bit on the generating machine).  On a machine with the same CPU model (manifest "cpu") the
oracle must reproduce them bit for bit (same ATen CPU ops in the same order); on another
CPU the fp32 GEMM kernels round differently, so the bar there is 1e-5 relative per step.
The synthetic meshes must also regenerate identically (digest check), since fixtures store
only the inputs that are not derivable.
"""
import hashlib

import numpy as np
import pytest
import torch

from conftest import golden, manifest, per_step_rel, weights
import msgnn_torch as orc
from mswegnn.mesh import make_multiscale_mesh, make_single_scale_mesh, wet_state, mesh_config


def _digest(g):
    h = hashlib.sha256()
    for k in ("x", "edge_index", "edge_attr", "edge_ptr", "node_ptr", "intra_mesh_edge_index",
              "intra_edge_ptr", "BC", "node_BC"):
        if k in g.keys():
            h.update(np.ascontiguousarray(getattr(g, k).numpy()).tobytes())
    return np.frombuffer(bytes.fromhex(h.hexdigest()), np.uint8)


@pytest.fixture(autouse=True)
def _threads():
    torch.set_num_threads(min(8, torch.get_num_threads()))


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


SAME_CPU = manifest().get("cpu") == _cpu_model()


def assert_pinned(ours, ref):
    """Bit-exact on the fixture's CPU model, 1e-5 relative per step elsewhere."""
    ref = torch.as_tensor(ref)
    if SAME_CPU:
        assert torch.equal(ours, ref), (ours - ref).abs().max().item()
    else:
        o, r = ours.reshape(ours.shape[0], -1, ours.shape[-1] if ours.dim() == 3 else 1), \
            ref.reshape(ref.shape[0], -1, ref.shape[-1] if ref.dim() == 3 else 1)
        assert per_step_rel(o, r) <= 1e-5


@pytest.mark.parametrize("ck", ["K4_F32", "K2_F16"])
def test_oracle_single_step(ck):
    fx = golden(f"fx_tiny_{ck}_step")
    cfg = manifest()[f"weights_{ck}_cfg"]
    g = wet_state(make_multiscale_mesh(**mesh_config("tiny"), T=48), seed=1)
    assert np.array_equal(_digest(g), fx["digest"]), "mesh generator drifted"
    y = orc.forward(weights(ck), cfg, g)
    assert_pinned(y, torch.from_numpy(fx["y"]))


@pytest.mark.parametrize("ck", ["K4_F32", "K2_F16"])
def test_oracle_rollout48(ck):
    fx = golden(f"fx_small_{ck}_rollout48")
    cfg = manifest()[f"weights_{ck}_cfg"]
    g = make_multiscale_mesh(**mesh_config("small"), T=48)
    assert np.array_equal(_digest(g), fx["digest"])
    r = orc.rollout(weights(ck), cfg, g)
    assert_pinned(r, torch.from_numpy(fx["rollout"]))


def test_oracle_f64_default_width():
    """config.yaml's default width F = 64 (mlp_layers 3, K 4; no shipped checkpoint: the
    reference's seeded initialisation, which the drop-in's seeded init reproduces): the oracle
    against the reference's single step, 48-step dry-start rollout and 8-step wet-start rollout
    (oracle/gen_golden_f64.py)."""
    from conftest import build_msgnn, state_dict_of
    cfg = manifest()["fx_F64_cfg"]
    cfg = {k: v for k, v in cfg.items() if k != "weights"}
    P = state_dict_of(build_msgnn(4, 64, 4))
    fx = golden("fx_tiny_F64_step")
    g = wet_state(make_multiscale_mesh(**mesh_config("tiny"), T=48), seed=1)
    assert np.array_equal(_digest(g), fx["digest"])
    assert_pinned(orc.forward(P, cfg, g), torch.from_numpy(fx["y"]))
    fx = golden("fx_small_F64_rollout48")
    g = make_multiscale_mesh(**mesh_config("small"), T=48)
    assert np.array_equal(_digest(g), fx["digest"])
    assert_pinned(orc.rollout(P, cfg, g), torch.from_numpy(fx["rollout"]))
    fx = golden("fx_small_F64_wet_rollout8")
    g = wet_state(make_multiscale_mesh(**mesh_config("small"), T=8), seed=4)
    assert np.array_equal(_digest(g), fx["digest"])
    assert_pinned(orc.rollout(P, cfg, g), torch.from_numpy(fx["rollout"]))


IRREGULAR = ["fx_irr_tiny_K4_F32_step", "fx_irr_small_K4_F32_rollout48", "fx_irr_small_K4_F32_wet_rollout8"]


def irregular_fixture(name):
    """-> (input graph rebuilt from the manifest's arguments, fixture arrays) of a fixture the
    reference wrote on an irregular, renumbered mesh (oracle/gen_golden_irregular.py)."""
    from mswegnn.mesh import irregularize
    spec = manifest()["fx_irr_spec"][name]
    g = make_multiscale_mesh(**mesh_config(spec["mesh"]), T=spec["T"])
    if spec["wet"] is not None:
        g = wet_state(g, seed=spec["wet"])
    g = irregularize(g, spec["seed"], order="canonical")[0]
    fx = golden(name)
    assert np.array_equal(_digest(g), fx["digest"]), "irregular mesh generator drifted"
    return g, fx


@pytest.mark.parametrize("name", IRREGULAR)
def test_oracle_irregular_mesh(name):
    """The reference's own forward / rollout_test (K4_F32) on irregularize()d meshes: 0..10
    children per coarse face, orphans, deleted finest faces, permuted ids."""
    g, fx = irregular_fixture(name)
    cfg = manifest()["weights_K4_F32_cfg"]
    if "y" in fx:
        assert_pinned(orc.forward(weights("K4_F32"), cfg, g), torch.from_numpy(fx["y"]))
    else:
        assert_pinned(orc.rollout(weights("K4_F32"), cfg, g), torch.from_numpy(fx["rollout"]))


def test_oracle_msgnn3_wet():
    fx = golden("fx_small3_msgnn3_wet")
    cfg = manifest()["weights_msgnn3_F32_seed666_cfg"]
    g = wet_state(make_multiscale_mesh(**mesh_config("small3"), T=6), seed=3)
    assert np.array_equal(_digest(g), fx["digest"])
    P = weights("msgnn3_F32_seed666")
    assert_pinned(orc.forward(P, cfg, g), torch.from_numpy(fx["y"]))
    assert_pinned(orc.rollout(P, cfg, g), torch.from_numpy(fx["rollout"]))


def test_oracle_gnn_config1():
    fx = golden("fx_gnn_small_rollout10")
    cfg = manifest()["weights_gnn_F32_seed42_cfg"]
    g = wet_state(make_single_scale_mesh(n_coarse=3, refinements=3, T=10), seed=2)
    assert np.array_equal(_digest(g), fx["digest"])
    P = weights("gnn_F32_seed42")
    assert_pinned(orc.forward(P, cfg, g), torch.from_numpy(fx["y"]))
    assert_pinned(orc.rollout(P, cfg, g), torch.from_numpy(fx["rollout"]))


def test_oracle_zenodo_size_rollout():
    """Config-2-sized mesh (N0 = 10,369; 4 scales; K4_F32), 48 steps, selected steps."""
    fx = golden("fx_zenodo4_K4_F32_rollout48")
    cfg = manifest()["weights_K4_F32_cfg"]
    g = make_multiscale_mesh(**mesh_config("zenodo4"), T=48)
    assert np.array_equal(_digest(g), fx["digest"])
    r = orc.rollout(weights("K4_F32"), cfg, g)
    assert_pinned(r[..., fx["steps"]], torch.from_numpy(fx["rollout_sel"]))


def test_oracle_dk15_first_steps():
    """Config 4 (dk15-like, T = 200): the oracle's first 20 steps against the reference's
    stored steps 0 and 19 (the GPU test checks every stored step up to 199)."""
    fx = golden("fx_dk15_K4_F32_rollout200")
    cfg = manifest()["weights_K4_F32_cfg"]
    g = make_multiscale_mesh(**mesh_config("dk15"), T=200)
    assert np.array_equal(_digest(g), fx["digest"])
    r = orc.rollout(weights("K4_F32"), cfg, g, 20)
    idx = [i for i, s in enumerate(fx["steps"]) if s < 20]
    assert_pinned(r[..., fx["steps"][idx]], torch.from_numpy(fx["rollout_sel"][..., idx]))


def test_oracle_upwind_mode_and_seeded_init():
    """upwind_mode=True on every processor (gnn.py:431-432), pinned to the reference's own
    rollout; the weights are the drop-in's seeded init (seed 666), so this also pins that
    construction order against the reference's."""
    from conftest import build_msgnn, state_dict_of
    fx = golden("fx_upwind_msgnn3_K2")
    cfg = manifest()["fx_upwind_msgnn3_K2_cfg"]
    g = wet_state(make_multiscale_mesh(n_coarse=2, num_scales=3, T=4), seed=11)
    assert np.array_equal(_digest(g), fx["digest"])
    m = build_msgnn(3, 32, 2)
    r = orc.rollout(state_dict_of(m), cfg, g)
    assert_pinned(r, torch.from_numpy(fx["rollout"]))


def test_oracle_on_reference_ingested_dataset():
    """fx_ingest: simulations in the reference's pickled-dataset layout prepared by the
    REFERENCE's own ingest (get_scalers, create_data_attr, to_temporal_dataset with config.yaml's
    dataset settings) and rolled out by its rollout_test (K4_F32, full 48-step test horizon);
    the oracle on the ingested arrays reproduces it, single graphs and the 2-graph batch."""
    from conftest import ingest_samples
    from mswegnn.batch import collate
    from mswegnn.rollout import adapt_batch_training
    samples, rb = ingest_samples()
    P = weights("K4_F32")
    cfg = orc.msgnn_config(num_scales=4, hid_features=32, K=4)
    for g, T, ref in samples:
        assert T == 48 and g.x.shape[1] == 8
        assert_pinned(orc.rollout(P, cfg, g, T), ref)
    b = adapt_batch_training(collate([g for g, _, _ in samples]))
    r = orc.rollout(P, cfg, b, samples[0][1])
    assert per_step_rel(r, rb) <= 1e-5  # batched CPU GEMMs block rows differently
