"""Kernel arguments pinned at kernel entry (kernels/k_base.h MSW_PIN) against the `lazyargs` build
variant (-DMSW_ARGS_HOIST=0: every field fetched where it is first used, the encoders' scale
search as a loop, the rollout I/O record read field by field through its pointer, no scheduling
barrier in the grid-stride last hop, k_edge_mlp's step increment at the kernel's top): the parent
commit's way of fetching arguments.  Only the order of loads differs, so every result is bit
for bit the same.

One child process per library (a process loads one; as test_build_variant_matches_default_bitwise):
the child runs every case below in fresh plans and prints a digest of each result and the
kernel variants each plan launched (EnginePlan.schedule()).  The meshes are the suite's
smallest, `tiny` and `small`, irregularised once.

cases = widths F = 16, 32, 64 and the padded width 50  x  forward, a 4-step rollout, a two-mesh
batch, on the default schedule; then at F = 32 and 64 once under MSW_GRID_CAP=2 (the grid-stride
kernels, the row-layout pool and hop), once with MSW_XCD_MAX=0 (the packing early return is one of
the hoisted branches), once as a 2-part decomposition; and one schedule per width that switches
on the kernels the small meshes' default schedules do not pick (split edge MLP, row epilogue,
feature-split hop, no cooperative kernels).  test_every_kernel_family_ran checks from the
schedules that, between them, the cases launched every kernel family that pins its arguments.

The module builds the lazyargs variant when it is missing or stale (build_engine.build, cached by
source hash).
"""
import hashlib
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 4
WIDTHS = (16, 32, 64, 50)
# schedule variants: name -> (MSW_* environment, widths)
SCHEDULES = {
    "default": ({}, WIDTHS),
    "cap2": ({"MSW_GRID_CAP": "2"}, (32, 64)),
    "xcd0": ({"MSW_XCD_MAX": "0"}, (32, 64)),
    "parts2": ({}, (32, 64)),
    # the kernels a small mesh's default schedule leaves out
    "other": ({"MSW_SPLIT_EDGE_MLP": "1", "MSW_EPI_SPLIT_TILES": "1", "MSW_HOP_SPLIT": "1", "MSW_COOP_WAVES": "0",
               "MSW_ENC_COOP": "0", "MSW_POOL_FUSE": "0", "MSW_UNPOOL_FUSE": "0", "MSW_DEFER_DECODE": "0"}, WIDTHS),
    "other cap2": ({"MSW_GRID_CAP": "2", "MSW_COOP_WAVES": "0", "MSW_ENC_COOP": "0", "MSW_HOP_ROWS": "0",
                    "MSW_HOP_SPLIT": "0", "MSW_EPI_SPLIT_TILES": "1", "MSW_POOL_FUSE": "0"}, (32, 64)),
}
CASES = [(s, F) for s, (_, ws) in SCHEDULES.items() for F in ws]
RUNS = ("forward", "rollout", "batch")

# schedule variant name (k_pick.h pick_name) -> kernel family, by (prefix, nt or None)
FAMILIES = ["k_hop", "k_hop_rows", "k_hop_split", "k_hop_coop", "k_edge_hop", "k_edge_coop", "k_edge_coop4",
            "k_edge_mlp", "k_encode", "k_encode_coop", "k_decode_fwd", "k_pool", "k_pool_edge", "k_epi"]


def family(variant, nt):
    if variant == "exchange":  # a decomposition's halo copies: not a step kernel
        return None
    for prefix, fam in (("hop rows", "k_hop_rows"), ("hop split", "k_hop_split"), ("hop coop", "k_hop_coop"),
                        ("hop", "k_hop"), ("edge_hop", "k_edge_hop"), ("edge_mlp", "k_edge_mlp"),
                        ("edge_coop2", "k_edge_coop4" if nt == 4 else "k_edge_coop"), ("edge_coop4", "k_edge_coop4"),
                        ("encode coop", "k_encode_coop"), ("encode", "k_encode"), ("decode", "k_decode_fwd"),
                        ("pool rows", "k_pool"), ("pool edge", "k_pool_edge"), ("epi", "k_epi")):
        if variant == prefix or variant.startswith(prefix + " "):
            return fam
    raise AssertionError(f"unknown schedule variant {variant!r}")


# ------------------------------------------------------------------------------------ child
def _digest(t):
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def _child():
    """Runs every case with the library MSW_LIB_VARIANT names; one JSON line of results."""
    sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "mswe-gnn_amd"), os.path.join(ROOT, "oracle")]
    import copy

    import torch
    from conftest import build_msgnn
    from mswegnn.batch import collate
    from mswegnn.engine import EnginePlan, plan_for
    from mswegnn.rollout import adapt_batch_training, rollout_test
    from test_irregular_mesh import GPU_SEEDS, irregular

    cuda = torch.device("cuda", 0)
    gs = [irregular("small", GPU_SEEDS[0], wet=4, T=T)[0], irregular("tiny", GPU_SEEDS[1], wet=5, T=T)[0]]
    out = {}
    for sched, F in CASES:
        env = SCHEDULES[sched][0]
        for k in [k for k in os.environ if k.startswith("MSW_") and k != "MSW_LIB_VARIANT"]:
            del os.environ[k]
        os.environ.update(env)
        m = build_msgnn(4, F, 4, seed=100 + F).to(cuda)
        g = gs[0].to(cuda)
        res = {"variants": []}
        if sched == "parts2":
            from mswegnn.partition import PartitionedRollout
            pr = PartitionedRollout(m, g, 2, cuda)
            try:
                for pl in pr.plans:
                    res["variants"] += [[s["variant"], s["nt"]] for s in pl.schedule()]
                res["rollout"] = _digest(pr.rollout(g.x, g.BC, g.node_BC, g.type_BC, T))
            finally:
                pr.close()
        else:
            plan = EnginePlan(m, g, cuda)
            try:
                res["variants"] += [[s["variant"], s["nt"]] for s in plan.schedule()]
                res["variants"] += [[s["variant"], s["nt"]] for s in plan.schedule(rollout=False)]
                res["forward"] = _digest(plan.forward(g.x))
                res["rollout"] = _digest(plan.rollout(g.x, g.BC, g.node_BC, g.type_BC, T))
            finally:
                plan.close()
            mb = copy.deepcopy(m)
            mb.engine = "hip"
            batch = collate(gs).to(cuda)
            res["batch"] = _digest(rollout_test(mb, batch))
            res["variants"] += [[s["variant"], s["nt"]] for s in plan_for(mb, adapt_batch_training(batch)).schedule()]
        out[f"{sched}/{F}"] = res
    print(json.dumps(out))


# ------------------------------------------------------------------------------------ tests
_results = {}


def _library(variant):
    if variant not in _results:
        env = {k: x for k, x in os.environ.items() if not k.startswith("MSW_")}
        if variant:
            env["MSW_LIB_VARIANT"] = variant
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True,
                           env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        _results[variant] = json.loads(r.stdout.strip().splitlines()[-1])
    return _results[variant]


@pytest.fixture(scope="module")
def both():
    # the variant is built here when it is missing or stale (cached by source hash, as the default
    # library is by __graft_entry__.build()); a failed build fails the tests
    sys.path.insert(0, os.path.join(ROOT, "mswe-gnn_amd"))
    import build_engine
    if not (os.path.exists(build_engine.lib_path("lazyargs")) and build_engine.library_matches_sources("lazyargs")):
        build_engine.build(verbose=False, variant="lazyargs")
    return _library(""), _library("lazyargs")


@pytest.mark.parametrize("sched,F", CASES, ids=[f"{s.replace(' ', '_')}-F{F}" for s, F in CASES])
def test_pinned_arguments_match_lazy_bitwise(both, sched, F):
    pinned, lazy = both[0][f"{sched}/{F}"], both[1][f"{sched}/{F}"]
    runs = ("rollout",) if sched == "parts2" else RUNS
    for what in runs:
        assert pinned[what] == lazy[what], f"{what} differs between the default and the lazyargs library ({sched}, F {F})"
    assert pinned["variants"] == lazy["variants"], "the two libraries picked different schedules"


def test_every_kernel_family_ran(both):
    """Between them, the cases launched every kernel family that pins its arguments (step
    kernels of kernels/k_pick.h), and the schedule variants did what they are there for."""
    ran = {}
    for key, res in both[0].items():
        for variant, nt in res["variants"]:
            if family(variant, nt):
                ran.setdefault(family(variant, nt), set()).add(key)
    missing = [f for f in FAMILIES if f not in ran]
    assert not missing, f"no case launched {missing}; launched: { {f: sorted(k)[:3] for f, k in ran.items()} }"
    print({f: sorted(k) for f, k in ran.items()})
    cap = [v for key in ("cap2/32", "other cap2/32") for v, _ in both[0][key]["variants"]]
    assert any(" loop" in v for v in cap) and "hop rows" in cap and any(v.startswith("pool rows") for v in cap), cap


if __name__ == "__main__":
    if "--child" in sys.argv:
        _child()
