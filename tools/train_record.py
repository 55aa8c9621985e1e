"""The training kernels' buffer layout, and a digest of every tensor they return, under the library this
process loads.

Run once per library (MSW_LIB_VARIANT=<name> selects lib/libmswegnn_<name>.so), each in a process of its
own, and compare the two files byte for byte: a refactor of csrc/train.hip or mswegnn/autograd.py must
leave them equal (the kernels use no atomics and fix every summation order, so a differing digest is a
changed value, not noise).
    python tools/train_record.py --out profiles/train_dedup/record.txt [--host-only]

Host section (no GPU needed; --host-only stops after it): saved_floats and scratch_floats of every
descriptor of tests/test_host_cpu.py's train_layout_table through msw_mlp_train_workspace /
msw_swegnn_train_workspace.

Device section: for every name of tests/train_cases.py's MLP_SPECS, SWEGNN_SPECS and POOL_SPECS, the
sha256 (first 16 hex digits) of the bytes of every tensor mlp_apply / swegnn_apply / pool_apply and their
backward return -- on the planted data, and on the full-precision data (random normal inputs, the
transcendental activations in turn, normalize=True), built as tests/test_gpu_train_exact.py builds them;
then the output and every parameter gradient of one MSGNN training step, set up as
tests/test_gpu_train.py::test_msgnn_training_step_gradients.
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "mswe-gnn_amd"), os.path.join(ROOT, "oracle")]


def digests(res):
    """name -> tensor (or None) as 'name=digest' in name order."""
    out = []
    for k in sorted(res):
        t = res[k]
        out.append(f"{k}=" + ("none" if t is None else
                              hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]))
    return " ".join(out)


def host_section():
    from mswegnn import _lib as L
    from test_host_cpu import train_layout_table
    lib = L.lib()
    lines = ["# host: descriptor: saved_floats scratch_floats"]
    for label, d in train_layout_table():
        s, t = C.c_int64(-1), C.c_int64(-1)
        fn = lib.msw_mlp_train_workspace if isinstance(d, L.MswMlpTrainDesc) else lib.msw_swegnn_train_workspace
        L.check(fn(C.byref(d), C.byref(s), C.byref(t)))
        lines.append(f"{label}: {s.value} {t.value}")
    return lines


def device_section():
    import torch
    import train_cases as tc
    import test_gpu_train_exact as ex
    from conftest import build_msgnn, weights
    from models.gnn import SWEGNN
    from mswegnn.mesh import make_multiscale_mesh, mesh_config, wet_state
    from test_gpu_train_fuzz import _grads
    cuda = torch.device("cuda", 0)
    lines = ["# device: family data case: tensor=sha256[:16] ..."]
    for i, name in enumerate(tc.MLP_SPECS):
        lines.append(f"mlp planted {name}: " + digests(ex.hip_mlp(tc.mlp_case(name), cuda)))
        case = tc.mlp_case(name, False)
        layers = ex._smooth_layers(case, i)
        res = ex.hip_mlp(dict(case, layers=layers), cuda, ex._smooth_seq(layers, torch.float32).to(cuda))
        lines.append(f"mlp full {name}: " + digests(res))
    for i, name in enumerate(tc.SWEGNN_SPECS):
        lines.append(f"swegnn planted {name}: " + digests(ex.hip_swegnn(tc.swegnn_case(name), cuda)))
        case, sp = tc.swegnn_case(name, False), tc.SWEGNN_SPECS[name]
        torch.manual_seed(tc.hash_name(name))
        lay = SWEGNN(sp["F"], sp["F"], sp["ef"], K=sp["K"], normalize=True, with_filter_matrix=sp["filt"],
                     with_gradient=sp["grad"], upwind_mode=sp["upwind"], n_layers=sp["depth"],
                     activation=ex.SMOOTH[i % len(ex.SMOOTH)], bias=sp["bias"]).to(cuda)
        t = lambda a: torch.from_numpy(a).to(torch.float32).to(cuda) if a is not None else None  # noqa: E731
        res = _grads(lay, t(case["x_s"]), t(case["x_d"]), torch.from_numpy(case["edge_index"]).to(cuda),
                     t(case["edge_attr"]) if sp["ef"] else None, t(case["grad_out"]), "auto")
        lines.append(f"swegnn full {name}: " + digests(res))
    for name in tc.POOL_SPECS:
        for data, planted in (("planted", True), ("full", False)):
            lines.append(f"pool {data} {name}: " + digests(ex.hip_pool(tc.pool_case(name, planted), cuda)))
    g = wet_state(make_multiscale_mesh(**mesh_config("tiny"), T=4), seed=1).to(cuda)
    m = build_msgnn(4, 32, 4, state=weights("K4_F32")).to(cuda)
    m.train()
    m.engine = "auto"
    tgt = torch.rand(g.num_nodes, 2, device=cuda, generator=torch.Generator(cuda).manual_seed(7))
    m.zero_grad(set_to_none=True)
    y = m(g)
    ((y - tgt) ** 2).mean().backward()
    lines.append("msgnn step: " + digests({"y": y, **{n: p.grad for n, p in m.named_parameters()}}))
    torch.cuda.synchronize()
    from mswegnn import autograd as ag
    assert min(ag.MLP_CALLS[0], ag.POOL_CALLS[0], ag.SWEGNN_CALLS[0]) > 0, "the HIP training kernels did not run"
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--host-only", action="store_true")
    a = ap.parse_args()
    lines = host_section()
    if not a.host_only:
        lines += device_section()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    from mswegnn import _lib as L
    print(f"{a.out}: {len(lines)} lines under {os.path.basename(L.LIB_PATH)}")


if __name__ == "__main__":
    main()
