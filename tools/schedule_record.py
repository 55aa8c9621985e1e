"""Every launch of every schedule, and a digest of every result, under the library this process loads.

Run once per library (MSW_LIB_VARIANT=<name> selects lib/libmswegnn_<name>.so), each in a process
of its own, and compare the two files byte for byte: a host-side refactor must leave them equal.
    python tools/schedule_record.py --out profiles/plan_split/schedules.txt

The cases, meshes and switches are those of tests/test_gpu_args_hoist.py (widths 16 / 32 / 64 / 50 x
forward, rollout and a two-mesh batch on the default schedule, under MSW_GRID_CAP, without XCD
packing, as a 2-part decomposition, and with the switches that bring in the remaining kernels), then
the plans of the zenodo4, zenodo4_f64 and config3 workloads of bench.py.  For each: every field of
every EnginePlan.schedule() record of the rollout and the forward schedule, and the sha256 of each
forward, rollout and batch result.  Written as a table of the distinct launch records, then each
schedule as the numbers of its launches' records.
"""
import argparse
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "mswe-gnn_amd"), os.path.join(ROOT, "oracle")]

FIELDS = ("kind", "variant", "nt", "scale", "prelu", "grid", "waves", "units", "per_wg", "iters", "ragged", "lds")
WORKLOADS = ("zenodo4", "zenodo4_f64", "config3")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    out_path = ap.parse_args().out
    import torch
    from conftest import build_msgnn
    from mswegnn.batch import collate
    from mswegnn.engine import EnginePlan, plan_for
    from mswegnn.partition import PartitionedRollout
    from mswegnn.rollout import adapt_batch_training, rollout_test
    from test_gpu_args_hoist import CASES, SCHEDULES, T, _digest
    from test_irregular_mesh import GPU_SEEDS, irregular
    import bench

    cuda = torch.device("cuda", 0)
    records, body = {}, []

    def sched(label, plan):
        for name, rollout in (("rollout", True), ("forward", False)):
            ids = []
            for s in plan.schedule(rollout=rollout):
                assert tuple(s) == FIELDS, tuple(s)
                ids.append(records.setdefault(",".join(str(s[f]) for f in FIELDS), len(records)))
            body.append(f"{label}{name}: " + " ".join(map(str, ids)))

    def clean_env(env):
        for k in [k for k in os.environ if k.startswith("MSW_") and k != "MSW_LIB_VARIANT"]:
            del os.environ[k]
        os.environ.update(env)

    gs = [irregular("small", GPU_SEEDS[0], wet=4, T=T)[0], irregular("tiny", GPU_SEEDS[1], wet=5, T=T)[0]]
    for case, F in CASES:
        clean_env(SCHEDULES[case][0])
        body.append(f"# case {case}/{F}")
        m = build_msgnn(4, F, 4, seed=100 + F).to(cuda)
        g = gs[0].to(cuda)
        if case == "parts2":
            pr = PartitionedRollout(m, g, 2, cuda)
            try:
                for i, pl in enumerate(pr.plans):
                    sched(f"part{i} ", pl)
                body.append("sha256 rollout " + _digest(pr.rollout(g.x, g.BC, g.node_BC, g.type_BC, T)))
            finally:
                pr.close()
            continue
        plan = EnginePlan(m, g, cuda)
        try:
            sched("", plan)
            body.append("sha256 forward " + _digest(plan.forward(g.x)))
            body.append("sha256 rollout " + _digest(plan.rollout(g.x, g.BC, g.node_BC, g.type_BC, T)))
        finally:
            plan.close()
        mb = copy.deepcopy(m)
        mb.engine = "hip"
        batch = collate(gs).to(cuda)
        body.append("sha256 batch " + _digest(rollout_test(mb, batch)))
        sched("batch ", plan_for(mb, adapt_batch_training(batch)))
    clean_env({})
    for name in WORKLOADS:
        body.append(f"# workload {name}")
        g, m, _, _ = bench.build_workload(name, 0, T)
        g, m = g.to(cuda), m.to(cuda)
        plan = EnginePlan(m, g, cuda)
        try:
            sched("", plan)
            body.append("sha256 forward " + _digest(plan.forward(g.x)))
            body.append("sha256 rollout " + _digest(plan.rollout(g.x, g.BC, g.node_BC, g.type_BC, T)))
        finally:
            plan.close()
    torch.cuda.synchronize()
    head = ["# Every field of every launch of every schedule: a table of the distinct launch records, then each",
            "# schedule as the numbers of its launches' records, in launch order, and the sha256 of the results.",
            "# record: " + ",".join(FIELDS)]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(head + [f"L{i} {r}" for r, i in records.items()] + body) + "\n")
    print(f"{out_path}: {sum(len(b.split(': ')[1].split()) for b in body if ': ' in b)} launches, "
          f"{len(records)} distinct records")


if __name__ == "__main__":
    main()
