#!/usr/bin/env python3
"""Compare two directories of `hipcc --cuda-device-only -S` outputs kernel by kernel: python tools/isa_cmp.py BEFORE AFTER [RE=REPL]

Per kernel instance: whether the instruction text is identical, and instructions / VGPRs / SGPRs / scratch bytes before
and after (a kernel's text runs from its label to .Lfunc_end, comments and directives stripped; registers and scratch
come from the `.set <kernel>.num_vgpr / .numbered_sgpr / .private_seg_size` lines).  RE=REPL: a regex substitution applied to
BEFORE's mangled names, to pair kernels whose template arguments changed (gemm_f32_kernelILi1E=gemm_f32_kernelI)."""
import os, re, subprocess, sys


def kernels(path):
    txt, out = open(path).read(), {}
    for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)^\.Lfunc_end", txt, re.M | re.S):
        body = [re.sub(r"\.LBB\d+_", ".LBB_", l.split(";")[0].strip()) for l in m.group(2).splitlines()]  # (labels carry the function's index in its unit)
        body = [l for l in body if l and not l.startswith(".") and not l.endswith(":")]
        res = [int(re.search(r"\.set %s\.%s, (\d+)" % (m.group(1), k), txt).group(1)) for k in ("num_vgpr", "numbered_sgpr", "private_seg_size")]
        out[m.group(1)] = (body, [len(body)] + res)
    return out


before, after = sys.argv[1], sys.argv[2]
print("%-64s %-9s %15s %11s %11s %11s" % ("kernel", "text", "instructions", "VGPRs", "SGPRs", "scratch"))
for f in sorted(os.listdir(before)):
    if not f.endswith(".s") or not os.path.exists(os.path.join(after, f)): continue
    a, b = kernels(os.path.join(before, f)), kernels(os.path.join(after, f))
    if len(sys.argv) > 3:
        a = {re.sub(*sys.argv[3].split("=", 1), k): v for k, v in a.items()}
    for k in sorted(set(a) | set(b)):
        name = subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip().replace("mtgv::", "").replace("void ", "")
        if k not in a or k not in b:
            print("%-64s %s" % (f[:-2] + " " + name.split("(")[0], "only before" if k in a else "only after"))
            continue
        print("%-64s %-9s" % (f[:-2] + " " + name.split("(")[0], "identical" if a[k][0] == b[k][0] else "differs") +
              "".join(" %*d -> %-*d" % (w, x, w, y) for w, x, y in zip((6, 4, 4, 4), a[k][1], b[k][1])))
