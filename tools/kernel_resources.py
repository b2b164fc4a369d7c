#!/usr/bin/env python3
"""Print VGPR / SGPR / scratch / occupancy per kernel of the given units of csrc/ (hipcc -Rpass-analysis).

    tools/kernel_resources.py [unit.hip ...] [extra hipcc flags]

The compile line of a unit is the one csrc/Makefile would run for its object (`make -n`), so the per-unit flags (MARCH_EXTRA,
CALL_EXTRA, MARCH_RA / TRACE_RA, ...) are the shipped library's by construction."""
import re
import shlex
import subprocess
import sys
import os
import tempfile

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
csrc = os.path.join(root, "atm-raytracer_amd", "csrc")
units = [a for a in sys.argv[1:] if a.endswith(".hip")] or ["atmrt_kernels.hip", "atmrt_paths.hip", "atmrt_march_linear.hip"]
flags = [a for a in sys.argv[1:] if not a.endswith(".hip")]


def compile_line(unit, obj_out):
    """the Makefile's own command for <unit>.o, writing to obj_out instead"""
    obj = unit[:-len(".hip")] + ".o"
    dry = subprocess.run(["make", "-n", "-W", unit, obj], cwd=csrc, capture_output=True, text=True, check=True).stdout
    lines = [l for l in dry.splitlines() if unit in l and " -c " in l]
    if len(lines) != 1:
        sys.exit(f"kernel_resources: `make -n {obj}` gave no single compile line for {unit}:\n{dry}")
    cmd = shlex.split(lines[0])
    cmd[cmd.index("-o") + 1] = obj_out
    return cmd


def without_parameters(name):
    """a demangled function name without its parameter list (template arguments may hold parentheses: `<(atmrt::SlotLayout)0>`)"""
    depth = 0
    for i in range(len(name) - 1, -1, -1):
        depth += (name[i] == ")") - (name[i] == "(")
        if depth == 0:
            return name[:i] if name[i] == "(" else name
    return name


out = ""
with tempfile.TemporaryDirectory() as tmp:
    for unit in units:
        cmd = compile_line(unit, os.path.join(tmp, "unit.o")) + ["-Rpass-analysis=kernel-resource-usage"] + flags
        run = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
        if run.returncode:
            sys.exit(run.stderr)
        out += run.stderr
cur, rows = None, {}
for line in out.splitlines():
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        cur = without_parameters(subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip())
        rows[cur] = {}
        continue
    m = re.search(r"remark:\s+([A-Za-z][^:]*): (\S+)", line)
    if m and cur:
        rows[cur][m.group(1).strip()] = m.group(2)
for k, v in rows.items():
    print(f"{k:42s} VGPR {v.get('VGPRs','?'):>4} AGPR {v.get('AGPRs','?'):>3} SGPR {v.get('TotalSGPRs','?'):>4} "
          f"scratch {v.get('ScratchSize [bytes/lane]','?'):>5} occ {v.get('Occupancy [waves/SIMD]','?'):>2} "
          f"LDS {v.get('LDS Size [bytes/block]','?')}")
