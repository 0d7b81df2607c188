#!/usr/bin/env python3
"""Kernel-resource table of core_amd/csrc/yk_device.hip, from the compiler's
own report (-Rpass-analysis=kernel-resource-usage), with the library's build
flags. No GPU is needed.

  tools/kernel_resources.py table [SRC]       print one line per kernel
  tools/kernel_resources.py diff OLD NEW      compare two saved tables

Kernel names are demangled, and the trailing template argument GL (the scene's
glossy level: kGLNone 0, kGLGlossy 1, kGLCoated 2, kGLGlass 3) is listed the way the
tables in profiles/ have listed it since it was a flag: dropped where it is 0
(or `false`), its default, and `true` where it is 1. The table lists
k_shade_primary<false, 0, false, 0> as k_shade_primary<false, 0, false>,
k_shade_primary<false, 0, false, 1> as k_shade_primary<false, 0, false, true>
and k_photon_hit<0> as k_photon_hit, so tables from before and after a kernel
gained the argument, or the argument became a level, line up.
"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
         "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-gpu-rdc", "-Wno-unused-result",
         "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", "-o", os.devnull]
FIELDS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill",
          "VGPRs Spill", "LDS Size [bytes/block]"]
# template arity, GL included, of the kernels whose last template argument is GL
GL_ARITY = {"k_shade_primary": 4, "k_shade_bounce": 3, "k_path_start": 2, "k_fg_start": 2, "k_fg_hit": 2,
            "k_photon_hit": 1, "k_pm_post": 1, "k_pm_finish": 1, "k_pt_caustic": 1, "k_spawn": 1}


# kernels with a trailing light level XL after that (kXLNone 0 ... kXLSun 3), and their arity with it: a 0
# is dropped first, so that the instantiations from before the argument keep their names
XL_ARITY = {"k_fg_hit": 3, "k_photon_emit": 1}


def short_name(mangled):
    dem = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
    name = re.sub(r"^void ", "", dem)
    name = re.sub(r"\(.*$", "", name.replace("(anonymous namespace)::", "")).replace("yk::", "")
    m = re.match(r"(\w+)<(.*)>$", name)
    if m and (m.group(1) in GL_ARITY or m.group(1) in XL_ARITY):
        args = [a.strip() for a in m.group(2).split(",")]
        if len(args) == XL_ARITY.get(m.group(1)) and args[-1] == "0":
            args.pop()
            name = f"{m.group(1)}<{', '.join(args)}>" if args else m.group(1)
        # GL became a level (0 none, 1 glossy, 2 coated glossy): 0 and 1 print as the flag's false and true did
        if len(args) == GL_ARITY.get(m.group(1)) and args[-1] in ("false", "0"):
            name = f"{m.group(1)}<{', '.join(args[:-1])}>" if len(args) > 1 else m.group(1)
        elif len(args) == GL_ARITY.get(m.group(1)) and args[-1] == "1":
            name = f"{m.group(1)}<{', '.join(args[:-1] + ['true'])}>"
    return name


def table(src):
    hipcc = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    r = subprocess.run([hipcc] + FLAGS + [src], capture_output=True, text=True, cwd=os.path.join(ROOT, "core_amd"))
    if r.returncode:
        sys.exit(r.stderr[-4000:])
    rows, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass", line)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2)
        if k == "Function Name":
            cur = rows.setdefault(short_name(v), {})
        elif cur is not None and k in FIELDS:
            cur[k] = v
    out = ["# kernel | " + " | ".join(FIELDS)]
    for name in sorted(rows):
        out.append(name + " | " + " | ".join(rows[name].get(f, "?") for f in FIELDS))
    return "\n".join(out)


def load(path):
    rows = {}
    for line in open(path):
        if line.startswith("#") or "|" not in line:
            continue
        name, rest = line.split(" | ", 1)
        rows[name.strip()] = rest.strip()
    return rows


def main():
    if len(sys.argv) >= 2 and sys.argv[1] == "table":
        print(table(sys.argv[2] if len(sys.argv) > 2 else "csrc/yk_device.hip"))
        return 0
    if len(sys.argv) == 4 and sys.argv[1] == "diff":
        old, new = load(sys.argv[2]), load(sys.argv[3])
        bad = [k for k in old if new.get(k) != old[k]]
        for k in bad:
            print(f"CHANGED {k}\n  old {old[k]}\n  new {new.get(k, '(missing)')}")
        for k in sorted(set(new) - set(old)):
            print(f"NEW     {k} | {new[k]}")
        print(f"{len(old)} kernels of the old table, {len(bad)} changed, {len(set(new) - set(old))} new")
        return 1 if bad else 0
    sys.exit(__doc__)


if __name__ == "__main__":
    sys.exit(main())
