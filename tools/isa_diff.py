#!/usr/bin/env python3
"""Per-kernel comparison of the device assembly of two builds (no GPU needed):

    for f in scan le packet sort survey hop synth; do
        hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden -x hip --cuda-device-only -S \
              libbtbb_amd/csrc/$f.hip -o DIR/$f.s
    done                                   # once per build, into two directories
    tools/isa_diff.py OLD_DIR NEW_DIR > profiles/<set>/isa_diff.json

A kernel's body is compared after comments, file / line directives and the numbers of local labels are removed.  Prints one
JSON object: per file and kernel "identical" or the instruction counts and register / LDS / scratch figures of both builds;
exit status 1 when any kernel differs or exists on one side only."""
import json
import os
import re
import sys


def kernels(path):
    """{kernel name: (normalised instruction lines, resource figures from the code-object metadata)}"""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        name, body = m.group(1), []
        for line in m.group(2).split("\n"):
            line = re.sub(r"\.L(BB|tmp|func_begin)\d+(_\d+)?", lambda x: ".L" + x.group(1) + (x.group(2) or ""), line.split(";")[0]).strip()
            if line and not re.match(r"\.(file|loc|cfi_|p2align|Ltmp)", line):
                body.append(re.sub(r"\s+", " ", line))
        out[name] = [body, {}]
    for m in re.finditer(r"^  - \.agpr_count:.*?\n(.*?)\.wavefront_size:", text, re.S | re.M):
        meta = dict(re.findall(r"\.(\w+):\s+(\S+)", m.group(0)))
        if meta.get("name") in out:
            out[meta["name"]][1] = {k: int(meta[k]) for k in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                                                             "group_segment_fixed_size", "private_segment_fixed_size")}
    return out


def main(old_dir, new_dir):
    report, differs = {}, False
    for f in sorted(os.listdir(old_dir)):
        if not f.endswith(".s"):
            continue
        old, new = kernels(os.path.join(old_dir, f)), kernels(os.path.join(new_dir, f))
        rows = {}
        for name in sorted(set(old) | set(new)):
            if name not in old or name not in new:
                rows[name] = "only in the " + ("old" if name in old else "new") + " build"
            elif old[name][0] == new[name][0]:
                rows[name] = "identical"
            else:
                is_instr = lambda l: not l.startswith(".") and not l.endswith(":")          # noqa: E731
                rows[name] = {"instructions": [sum(map(is_instr, old[name][0])), sum(map(is_instr, new[name][0]))],
                              "old": old[name][1], "new": new[name][1]}
            differs |= rows[name] != "identical"
        report[f] = {"kernels": len(rows), "identical": sum(v == "identical" for v in rows.values()), "per_kernel": rows}
    json.dump(report, sys.stdout, indent=1)
    print()
    return 1 if differs else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
