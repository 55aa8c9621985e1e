"""Cost of a serial scalar round trip to the cold kernel-argument segment at kernel start.

Like tools/launch_floor.py: N dependent launches in one captured graph, replayed; the kernel is
a row gather (10,369 x 32 floats through a permutation) that reads the previous launch's
output.  Four forms of the same kernel (tools/kernarg_floor.hip) that differ only in how a wave
gets its arguments:

  lazy     408-byte struct by value, read at three dependent points (as k_hop did)
  pinned   the same struct, every field pinned at kernel entry (one round trip)
  preload  the entry fields as leading scalar parameters, preloaded into SGPRs
  pointer  a single pointer argument

(lazy - pinned) / 2 is the cost of one serial round trip; pinned - preload what the last one
costs; pointer is the floor of this gather.

usage: python tools/kernarg_floor.py [--n 35] [--reps 200] [--repeat 5] [--out FILE.json] [--build-only]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import time

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "kernarg_floor.hip")
LIB = os.path.join(HERE, "_bin", "kernarg_floor.so")
ARCH = os.environ.get("MSW_OFFLOAD_ARCH", "gfx950")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-shared", f"--offload-arch={ARCH}", "-mllvm", "-amdgpu-kernarg-preload-count=16"]
VARIANTS = ["lazy", "pinned", "preload", "pointer"]


def _hash():
    with open(SRC, "rb") as f:
        return hashlib.sha256(f.read() + " ".join(FLAGS).encode()).hexdigest()


def build():
    """Compile the micro-benchmark library unless it is there and matches the source."""
    try:
        with open(LIB + ".srchash") as f:
            if f.read().strip() == _hash() and os.path.exists(LIB):
                return LIB
    except OSError:
        pass
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    subprocess.run(["hipcc", *FLAGS, SRC, "-o", LIB], check=True)
    with open(LIB + ".srchash", "w") as f:
        f.write(_hash() + "\n")
    return LIB


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=35)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--build-only", action="store_true")
    a = ap.parse_args()
    lib = C.CDLL(build())
    if a.build_only:
        return
    lib.kf_run.restype = C.c_int
    lib.kf_run.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
    samples = {v: [] for v in VARIANTS}
    for _ in range(a.repeat):  # interleaved, so drift hits every variant alike
        for i, v in enumerate(VARIANTS):
            us = C.c_double()
            rc = lib.kf_run(i, a.n, a.reps, C.byref(us))
            if rc != 0:
                raise RuntimeError(f"kf_run({v}) failed: hipError {rc}")
            samples[v].append(us.value)
    med = {v: statistics.median(s) for v, s in samples.items()}
    res = {"launches_per_graph": a.n, "reps": a.reps, "rows": 10369, "feat": 32, "arg_bytes": 408,
           "us_per_launch_median": med, "us_per_launch_samples": samples,
           "us_per_round_trip": (med["lazy"] - med["pinned"]) / 2,
           "us_last_round_trip": med["pinned"] - med["preload"],
           "time": time.time()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
