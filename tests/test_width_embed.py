"""Zero-embedding of an F-wide model into a 64-wide one (CPU, oracle only).

The HIP engine runs hid_features 33..63 zero-padded to 64.  ``embed`` builds the model that
padding amounts to: every F-wide block of a weight or bias in the first F columns / rows of a
64-wide block, the rest zero.  With an activation for which f(0) = 0 the embedded twin computes
the native model's function: the pad columns of every feature row stay 0 and take part in
nothing.  This module checks that on the oracle (the summation order over 64 columns differs
from the one over F, so the two agree to rounding, not bit for bit); tests/test_gpu_width.py
then uses the twin to pin that the engine's padding is exactly this embedding.
"""
import pytest
import torch

from conftest import build_gnn, build_msgnn, per_step_rel, state_dict_of
import msgnn_torch as orc
from mswegnn.mesh import make_multiscale_mesh, make_single_scale_mesh, mesh_config, wet_state

T = 6
TWIN_TOL = 1e-6  # per step: fp32 rounding of re-associated sums (measured <= 1.4e-7)


def _embed_dim(t, dim, F, Fp):
    n = t.shape[dim]
    if n not in (F, 2 * F, 4 * F, 5 * F):
        return t
    nb = n // F
    shape = list(t.shape)
    shape[dim] = nb * Fp
    out = t.new_zeros(shape)
    for b in range(nb):
        out.narrow(dim, b * Fp, F).copy_(t.narrow(dim, b * F, F))
    return out


def embed(state, F, Fp):
    """Zero-embed an F-wide state dict into an Fp-wide one: each dimension equal to F, 2F, 4F
    or 5F maps block-wise to Fp, 2Fp, 4Fp or 5Fp (biases too); scalars (PReLU slopes),
    ``residual_weights`` and the 1/3/6-wide inputs and 2-wide outputs are left alone."""
    assert F > 6 and Fp >= F
    out = {}
    for k, v in state.items():
        t = v.detach().clone()
        if k != "residual_weights" and t.numel() > 1:
            for dim in range(t.dim()):
                t = _embed_dim(t, dim, F, Fp)
        out[k] = t
    return out


def msgnn_case(S, F, K, **kw):
    """-> (builder(hid, state=None), oracle cfg(hid)) of a seeded MSGNN."""
    return (lambda hid=F, state=None: build_msgnn(S, hid, K, state=state, **kw),
            lambda hid=F: orc.msgnn_config(num_scales=S, hid_features=hid, K=K, **kw))


def gnn_case(F, K=2, n_layers=2, mlp_layers=1, **kw):
    return (lambda hid=F, state=None: build_gnn(hid, K, n_layers, mlp_layers, state=state, **kw),
            lambda hid=F: orc.gnn_config(hid_features=hid, K=K, n_GNN_layers=n_layers, mlp_layers=mlp_layers, **kw))


def tiny_mesh(S, T=T, seed=3):
    """A wet `tiny` mesh with S scales (S = 1: its finest scale alone, for the GNN)."""
    if S == 1:
        return wet_state(make_single_scale_mesh(n_coarse=2, refinements=3, T=T), seed=seed)
    cfg = dict(mesh_config("tiny"), num_scales=S)
    return wet_state(make_multiscale_mesh(**cfg, T=T), seed=seed)


# name -> (scales, F, case)
CASES = {
    "F50_S4_K2": (4, 50, msgnn_case(4, 50, 2)),
    "F50_S3_K5": (3, 50, msgnn_case(3, 50, 5)),
    "F33_S2_K12": (2, 33, msgnn_case(2, 33, [1, 2])),
    "F63_S3_K3": (3, 63, msgnn_case(3, 63, 3)),
    "F40_relu": (3, 40, msgnn_case(3, 40, 2, mlp_activation="relu")),
    "GNN_F50_mlp2": (1, 50, gnn_case(50, mlp_layers=2)),
}


@pytest.fixture(autouse=True)
def _threads():
    torch.set_num_threads(min(8, torch.get_num_threads()))


@pytest.mark.parametrize("name", sorted(CASES))
def test_embedded_twin_matches_native(name):
    S, F, (build, cfg) = CASES[name]
    P = state_dict_of(build())
    P64 = embed(P, F, 64)
    twin = build(64, P64)  # strict=True: the embedded state is a 64-wide model's
    for k, v in twin.state_dict().items():
        assert torch.equal(v, P64[k]), k
    g = tiny_mesh(S)
    ref = orc.rollout(P, cfg(), g, T)
    got = orc.rollout(P64, cfg(64), g, T)
    wet = float((ref[:, 0, -1] > 0).float().mean())
    assert ref.abs().max() > 0.1 and wet > 0.1, (name, wet)
    e = per_step_rel(got, ref)
    print(f"{name}: embedded twin vs native, per-step rel {e:.2e} (wet fraction at the last step {wet:.2f})")
    assert e <= TWIN_TOL, (name, e)


def test_embed_leaves_small_dims_alone():
    _, F, (build, _) = CASES["F50_S4_K2"]
    P = state_dict_of(build())
    P64 = embed(P, F, 64)
    assert torch.equal(P64["residual_weights"], P["residual_weights"])
    w = P64["gnn_processor.0.edge_mlp.0.weight"]  # [2F, 5F] -> [128, 320]
    assert tuple(w.shape) == (128, 320)
    assert torch.equal(w[:50, 64:114], P["gnn_processor.0.edge_mlp.0.weight"][:50, 50:100])
    assert w[50:64].abs().max() == 0 and w[:, 50:64].abs().max() == 0 and w[:, 306:].abs().max() == 0
    assert tuple(P64["dynamic_node_encoder.0.weight"].shape) == (64, 6)
    assert tuple(P64["node_decoder.4.weight"].shape) == (2, 64)


def test_sigmoid_twin_is_not_the_native_model():
    """sigmoid(0) = 0.5: the twin's pad columns enter the norm of s_ij, so zero-embedding alone
    does not reproduce a sigmoid model -- the engine masks those columns in its kernels
    (tests/test_gpu_width.py holds it to the native model)."""
    build, cfg = msgnn_case(3, 40, 2, mlp_activation="sigmoid")
    P, g = state_dict_of(build()), tiny_mesh(3)
    d = per_step_rel(orc.rollout(embed(P, 40, 64), cfg(64), g, T), orc.rollout(P, cfg(), g, T))
    print(f"sigmoid twin vs native: per-step rel {d:.2e}")
    assert d > TWIN_TOL
