"""bench.py's command line: a plain run measures the headline figure and nothing else, --full
adds the other records, --dump-outputs writes what the last timed step returned.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REL_TOL, ROOT, per_step_rel
import msgnn_torch as orc

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _dir_bytes(path):
    return sum(os.path.getsize(os.path.join(path, f)) for f in os.listdir(path))


def test_dump_outputs_formats_and_size_limit(tmp_path):
    """bench.dump_outputs: float32 (float64 kept) .npy files; an array over the limit is
    written as the same seeded ascending sample of its rows in every call, the rows beside it,
    and the files together stay within the limit."""
    import bench
    t = torch.arange(1000 * 2 * 3, dtype=torch.float32).reshape(1000, 2, 3)
    rec = bench.dump_outputs(str(tmp_path / "whole"), {"rollout": t, "d": t[:5].double(), "h": t[:5].half()})
    assert rec["rollout"] == {"shape": [1000, 2, 3], "dtype": "float32", "sampled_rows": None}
    assert np.array_equal(np.load(tmp_path / "whole" / "rollout.npy"), t.numpy())
    assert np.load(tmp_path / "whole" / "d.npy").dtype == np.float64
    assert np.load(tmp_path / "whole" / "h.npy").dtype == np.float32
    assert sorted(os.listdir(tmp_path / "whole")) == ["d.npy", "h.npy", "rollout.npy"]
    limit = 16384  # of the 24,000-byte array: (16384 - headers) // (24 B row + 8 B index) rows
    for d in ("a", "b"):
        rec = bench.dump_outputs(str(tmp_path / d), {"rollout": t}, limit=limit)
        assert _dir_bytes(tmp_path / d) <= limit
    keep = (limit - bench.NPY_HEADERS_BYTES) // 32
    assert rec["rollout"]["sampled_rows"] == keep and rec["rollout"]["shape"] == [keep, 2, 3]
    rows = np.load(tmp_path / "a" / "rollout_rows.npy")
    assert rows.dtype == np.float64 and np.all(np.diff(rows) > 0) and len(rows) == keep
    a = np.load(tmp_path / "a" / "rollout.npy")
    assert np.array_equal(a, t.numpy()[rows.astype(np.int64)])
    assert np.array_equal(a, np.load(tmp_path / "b" / "rollout.npy"))
    assert np.array_equal(rows, np.load(tmp_path / "b" / "rollout_rows.npy"))
    assert bench.DUMP_LIMIT_BYTES == 64 * 10 ** 6


def _bench_line(monkeypatch, capsys, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_rollout(cuda, tmp_path, monkeypatch, capsys):
    """`bench.py --gpus 1 --steps K --warmup W` on the tiny workload: the line carries the
    headline figure (value = fine nodes x T / the step time ms_per_step of K timed steps) and
    none of the --full records; --dump-outputs writes the rollout the last timed step returned,
    float32 [all nodes, 2, T], identical from run to run and equal to the oracle's rollout of
    the same workload at the suite's fp32 bar."""
    import bench
    T = 4
    runs = []
    for d in ("a", "b"):
        runs.append(_bench_line(monkeypatch, capsys, "--gpus", "1", "--steps", "2", "--warmup", "1",
                                "--workload", "tiny", "--T", str(T), "--dump-outputs", str(tmp_path / d)))
    r = runs[0]
    assert r["steps"] == 2 and r["warmup"] == 1 and r["n_gpus"] == 1 and r["full"] is False
    assert r["unit"] == "fine-node-steps/s" and r["higher_is_better"] is True and r["dtype"] == "f32"
    assert r["ms_per_step"] > 0
    assert r["value"] == pytest.approx(r["config"]["fine_nodes"] * T / (r["ms_per_step"] * 1e-3), rel=1e-9)
    for k in ("roofline", "cpu_baseline", "parity", "caller_overhead", "strong_scaling"):
        assert k not in r, k
    g, m, w, desc = bench.build_workload("tiny", seed=0, T=T)
    assert r["dumped_outputs"] == {"rollout": {"shape": [desc["all_nodes"], 2, T], "dtype": "float32",
                                               "sampled_rows": None}}
    a, b = (np.load(tmp_path / d / "rollout.npy") for d in ("a", "b"))
    assert a.dtype == np.float32 and a.shape == (desc["all_nodes"], 2, T)
    assert np.array_equal(a, b)
    assert os.listdir(tmp_path / "a") == ["rollout.npy"]
    P = {k: v.detach() for k, v in m.state_dict().items()}
    ref = orc.rollout(P, orc.msgnn_config(num_scales=w["S"], hid_features=w["F"], K=w["K"]), g, T)
    assert per_step_rel(torch.from_numpy(a), ref) <= REL_TOL


@pytest.mark.gpu
def test_full_run_adds_the_other_records(cuda, monkeypatch, capsys):
    """--full on the default workload (the ~1M-node roofline and the CPU baseline switched off by
    their own options): the same headline fields plus the roofline record and the parity of the
    48-step rollout against the stored reference rollout."""
    r = _bench_line(monkeypatch, capsys, "--gpus", "1", "--steps", "1", "--warmup", "1", "--full",
                    "--no-roofline-large", "--no-cpu-baseline")
    assert r["full"] is True and r["steps"] == 1 and r["ms_per_step"] > 0
    assert r["config"]["workload"] == "zenodo4" and r["config"]["rollout_steps"] == 48
    assert r["roofline"]["avg_launch_us"] > 0 and r["roofline"]["bound"] == "hbm"
    assert "large_mesh" not in r["roofline"] and r["cpu_baseline"] is None
    assert r["parity"]["vs_reference_fixture"]["max_rel_err"] <= REL_TOL
    assert "dumped_outputs" not in r
