"""Registers per kernel of one HIP source file, from the compiler's own resource-usage remarks (needs hipcc, no GPU).

    python tools/kernel_resources.py attn_kernels.hip              # every build of the file in cosa_amd/build.py (plain and @f16)
    python tools/kernel_resources.py attn_kernels.hip@f16 x3 dq    # one build, kernels whose name contains "x3" or "dq"
    python tools/kernel_resources.py attn_kernels.hip --json       # machine-readable, to diff two trees

The file is compiled for the device only with the flags build.py gives it plus -Rpass-analysis=kernel-resource-usage; nothing is
written.  Per kernel: VGPRs, AGPRs, scratch bytes per lane, occupancy (waves per SIMD), SGPRs, LDS bytes per block.  Template
instances are listed with their arguments."""
import json
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cosa_amd import build

FIELDS = (("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "occupancy"),
          ("TotalSGPRs", "sgpr"), ("LDS Size [bytes/block]", "lds"), ("VGPRs Spill", "vgpr_spill"), ("SGPRs Spill", "sgpr_spill"))
REMARK = re.compile(r":\d+:\d+: remark:\s+(.*?):\s+(\S+)\s*(?:\[-Rpass-analysis=kernel-resource-usage\])?\s*$")


def parse_remarks(text):
    """[(mangled name, {field: int})] in the order of the remarks."""
    out, cur = [], None
    keys = dict(FIELDS)
    for line in text.splitlines():
        m = REMARK.search(line)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2)
        if k == "Function Name":
            cur = {}
            out.append((v, cur))
        elif cur is not None and k in keys and v.lstrip("-").isdigit():
            cur[keys[k]] = int(v)
    return out


TYPES = (("DF16b", "bf16"), ("DF16_", "fp16"), ("f", "float"), ("d", "double"), ("i", "int"), ("h", "uchar"))


def short_name(mangled):
    """kernel<args> of an Itanium-mangled kernel name (the namespaces and the parameter list dropped); the name itself if it is not one."""
    if not mangled.startswith("_Z"):
        return mangled
    i, ident = 2 + mangled.startswith("_ZN"), ""
    while i < len(mangled) and mangled[i].isdigit():
        j = i
        while mangled[j].isdigit():
            j += 1
        n = int(mangled[i:j])
        ident, i = mangled[j:j + n], j + n
    if i >= len(mangled) or mangled[i] != "I":
        return ident
    args, i = [], i + 1
    while i < len(mangled) and mangled[i] != "E":
        m = re.match(r"L([a-z])(n?\d+)E", mangled[i:])
        if m:
            v = m.group(2).replace("n", "-")
            args.append(("false", "true")[int(v) != 0] if m.group(1) == "b" else v)
            i += m.end()
            continue
        for code, name in TYPES:
            if mangled.startswith(code, i):
                args.append(name)
                i += len(code)
                break
        else:
            return ident + "<" + mangled[i:] + ">"
    return ident + "<" + ", ".join(args) + ">"


def resources(key):
    """Kernel resources of the build `key` of cosa_amd/build.py's SOURCES (e.g. "attn_kernels.hip@f16")."""
    src = key.partition("@")[0]
    cmd = [build._hipcc(), "-c", os.path.join(build.CSRC, src), "-o", os.devnull, "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage"] + build.COMMON + build.SOURCES[key]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed on " + key + "\n" + r.stderr[-4000:])
    rem = [(n, d) for n, d in parse_remarks(r.stderr) if "lds" in d]
    return [(short_name(n), d) for n, d in rem]


def main(argv):
    as_json = "--json" in argv
    argv = [a for a in argv if a != "--json"]
    if not argv:
        sys.exit(__doc__)
    name, filters = argv[0], argv[1:]
    keys = [name] if name in build.SOURCES and "@" in name else [k for k in build.SOURCES if k.partition("@")[0] == name]
    if not keys:
        sys.exit("no build of %s in cosa_amd/build.py (known: %s)" % (name, ", ".join(build.SOURCES)))
    result = {}
    for key in keys:
        rows = [(n, d) for n, d in resources(key) if not filters or any(f in n for f in filters)]
        result[key] = {n: d for n, d in rows}
        if as_json:
            continue
        print("%s  (%s)" % (key, " ".join(build.SOURCES[key]) or "no extra flags"))
        w = max([len(n) for n, _ in rows] + [6])
        print("  %-*s %5s %5s %8s %4s %5s %7s" % (w, "kernel", "VGPR", "AGPR", "scratch", "occ", "SGPR", "LDS"))
        for n, d in rows:
            print("  %-*s %5d %5d %8d %4d %5d %7d" % (w, n, d.get("vgpr", -1), d.get("agpr", -1), d.get("scratch", -1),
                                                      d.get("occupancy", -1), d.get("sgpr", -1), d.get("lds", -1)))
    if as_json:
        print(json.dumps(result, indent=1, sort_keys=True))


if __name__ == "__main__":
    main(sys.argv[1:])
