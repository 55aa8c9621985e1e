"""Kernel-argument census of the step kernels (host only, no GPU).

    python tools/kernarg_census.py [--csrc DIR] [--variant lazyargs] [--all] [-DNAME=VALUE ...]

Device-only compile (hipcc -S) of the three kernel translation units (kernels_nt1/2/4.hip),
cached by the sha256 of sources + flags under tools/_bin/kernarg_census/.  For every kernel of
the families a schedule can launch it prints

    argument-segment bytes, preload length (dwords), VGPRs, SGPRs, scratch bytes,
    the serial scalar-load round trips before the first vector memory load,
    the scalar loads after that load.

A "round trip" is a wait on the scalar/LDS counter (s_waitcnt ... lgkmcnt) with at least one
scalar load outstanding since the previous such wait, counted in text order from the kernel's
entry to its first vector memory load (global / buffer / flat).  The kernel-argument segment is
cold at every kernel start, so each of them is a dependent trip to memory before the wave's first
gather.  The tool matches load mnemonics and s_waitcnt only.
"""
import hashlib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "mswe-gnn_amd"))

UNITS = ["kernels_nt1.hip", "kernels_nt2.hip", "kernels_nt4.hip"]
# the kernels schedule_dispatch can launch (kernels/k_pick.h)
FAMILIES = ["k_hop", "k_hop_rows", "k_hop_split", "k_hop_coop", "k_edge_hop", "k_edge_coop", "k_edge_coop4",
            "k_edge_mlp", "k_encode", "k_encode_coop", "k_decode_fwd", "k_pool", "k_pool_edge", "k_epi"]
SCALAR_LOAD = ("s_load_", "s_buffer_load_")
VECTOR_LOAD = ("global_load_", "buffer_load_", "flat_load_")


def _flags(csrc, extra):
    import build_engine as be
    inc = os.path.join(os.path.dirname(os.path.dirname(csrc)), "include")
    return ["-O3", "-std=c++17", f"--offload-arch={be.ARCH}", "--cuda-device-only", "-S", "-I", inc, *extra]


def _hash(csrc, flags):
    h = hashlib.sha256()
    for d, _, files in sorted(os.walk(csrc)):
        for f in sorted(files):
            if f.endswith((".h", ".hip")):
                h.update(f.encode())
                with open(os.path.join(d, f), "rb") as fh:
                    h.update(fh.read())
    h.update(" ".join(flags).replace(csrc, "<csrc>").replace(os.path.dirname(os.path.dirname(csrc)), "<root>").encode())
    return h.hexdigest()[:16]


def compile_units(csrc=None, extra=()):
    """Paths of the three units' assembly, compiled (in parallel) unless cached."""
    csrc = os.path.abspath(csrc or os.path.join(ROOT, "mswe-gnn_amd", "csrc"))
    flags = _flags(csrc, list(extra))
    odir = os.path.join(HERE, "_bin", "kernarg_census", _hash(csrc, flags))
    os.makedirs(odir, exist_ok=True)
    outs = [os.path.join(odir, u[:-4] + ".s") for u in UNITS]
    cmds = [["hipcc", *flags, os.path.join(csrc, u), "-o", o + ".tmp"] for u, o in zip(UNITS, outs)
            if not os.path.exists(o)]
    jobs = max(1, min(len(cmds), int(os.environ.get("MAX_JOBS", "3")), 3))
    with ThreadPoolExecutor(jobs) as ex:
        for r in list(ex.map(lambda c: subprocess.run(c, check=False), cmds)):
            if r.returncode != 0:
                raise subprocess.CalledProcessError(r.returncode, r.args)
            os.replace(r.args[-1], r.args[-1][:-4])
    return outs


def _demangle(names):
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True)
            return r.stdout.split("\n")[:len(names)]
        except (OSError, subprocess.CalledProcessError):
            continue
    return list(names)


def _family(dem):
    m = re.match(r"(?:void )?msw::(k_\w+)", dem)
    return m.group(1) if m else None


def _short(dem):
    return re.sub(r"^void ", "", dem).replace("msw::", "").split("(")[0].replace("(bool)", "").replace("(int)", "")


def _body_stats(lines):
    """(round trips before the first vector load, scalar loads after it) of one kernel body."""
    trips = pending = after = 0
    seen_vec = False
    for l in lines:
        l = l.split(";")[0].strip()
        if not l or l.startswith(".") or l.endswith(":"):
            continue
        op = l.split()[0]
        if op.startswith(VECTOR_LOAD):
            seen_vec = True
        elif op.startswith(SCALAR_LOAD):
            if seen_vec:
                after += 1
            else:
                pending += 1
        elif op == "s_waitcnt" and not seen_vec and pending and ("lgkmcnt" in l or re.search(r"s_waitcnt\s+(0x)?[0-9a-f]+$", l)):
            trips += 1
            pending = 0
    return trips, after


def census_file(path):
    """{mangled name: record} for every kernel of one assembly file."""
    text = open(path).read()
    lines = text.split("\n")
    out = {}
    # bodies: "name:" ... ".Lfunc_endN:"
    i = 0
    starts = {}
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w+):", l)
        if m:
            starts[m.group(1)] = i
    # kernel descriptors: preload length
    preload = {}
    cur = None
    for l in lines:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if m:
            cur = m.group(1)
            preload[cur] = 0
        m = re.match(r"\s*\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)", l)
        if m and cur:
            preload[cur] = int(m.group(1))
    # metadata: one YAML map per kernel
    meta = text[text.find(".amdgpu_metadata"):]
    for blk in re.split(r"\n  - \.agpr_count:", meta)[1:]:
        def field(k, blk=blk):
            m = re.search(r"\." + k + r":\s+(\S+)", blk)
            return m.group(1) if m else None
        name = field("name")
        if name is None or name not in starts:
            continue
        s = starts[name]
        e = next(k for k in range(s + 1, len(lines)) if lines[k].startswith(".Lfunc_end"))
        trips, after = _body_stats(lines[s + 1:e])
        out[name] = {"kernarg": int(field("kernarg_segment_size")), "preload": preload.get(name, 0),
                     "vgpr": int(field("vgpr_count")), "sgpr": int(field("sgpr_count")),
                     "scratch": int(field("private_segment_fixed_size")),
                     "sgpr_spill": int(field("sgpr_spill_count") or 0), "vgpr_spill": int(field("vgpr_spill_count") or 0),
                     "trips": trips, "after": after}
    return out


def census(csrc=None, extra=(), all_kernels=False):
    """[(unit, kernel, family, record)] of the schedulable kernels (or all), sorted by name."""
    rows = []
    for unit, path in zip(UNITS, compile_units(csrc, extra)):
        recs = census_file(path)
        names = sorted(recs)
        for name, dem in zip(names, _demangle(names)):
            fam = _family(dem)
            if all_kernels or fam in FAMILIES:
                rows.append((unit[:-4], _short(dem), fam, recs[name]))
    rows.sort(key=lambda r: (r[0], r[1]))
    return rows


def format_rows(rows):
    out = [f"{'unit':12s} {'kernel':44s} {'kernarg':>7s} {'preload':>7s} {'vgpr':>5s} {'sgpr':>5s} {'scratch':>7s} "
           f"{'spill s/v':>9s} {'trips':>5s} {'after':>5s}"]
    for unit, k, _, r in rows:
        out.append(f"{unit:12s} {k:44s} {r['kernarg']:7d} {r['preload']:7d} {r['vgpr']:5d} {r['sgpr']:5d} "
                   f"{r['scratch']:7d} {r['sgpr_spill']:4d}/{r['vgpr_spill']:<4d} {r['trips']:5d} {r['after']:5d}")
    return "\n".join(out)


def parse_table(path):
    """{(unit, kernel): record} from a table written by this tool (the committed records)."""
    rec = {}
    with open(path) as f:
        for l in f:
            p = l.split()
            if len(p) < 10 or p[0] == "unit":
                continue
            sp = p[-3].split("/")
            rec[(p[0], " ".join(p[1:-8]))] = {"kernarg": int(p[-8]), "preload": int(p[-7]), "vgpr": int(p[-6]),
                                              "sgpr": int(p[-5]), "scratch": int(p[-4]), "sgpr_spill": int(sp[0]),
                                              "vgpr_spill": int(sp[1]), "trips": int(p[-2]), "after": int(p[-1])}
    return rec


if __name__ == "__main__":
    argv = sys.argv[1:]
    csrc = argv[argv.index("--csrc") + 1] if "--csrc" in argv else None
    extra = [a for a in argv if a.startswith("-D")]
    if "--variant" in argv and argv[argv.index("--variant") + 1] == "lazyargs":
        extra.append("-DMSW_ARGS_HOIST=0")
    print(format_rows(census(csrc, extra, "--all" in argv)))
