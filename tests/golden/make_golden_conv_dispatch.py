"""tests/golden/conv_dispatch_b16.json: the convolution kernels the library launched for every layer of
tools/step_layers.py at B = 16 on an MI355X, recorded BEFORE the kernel choice moved into csrc/conv_plan.h.

One kernel trace per (kind, layer list), nothing else traced, each run under its own time limit:

    rocprofv3 --kernel-trace -d DIR -o t -- python3 tools/bench_conv.py --eager --iters 1 --kind K --set S

for K in fwd, dgrad, wgrad and S in all, teacher640, student640 (the tool runs the frozen teacher's layers forward only, so
dgrad / wgrad of teacher640 launch nothing).  Then, with the nine result databases as DIR/<K>_<S>.db:

    python tests/golden/make_golden_conv_dispatch.py DIR

keeps, in launch order, one record per dispatch of a kd6d kernel (the runtime's buffer copies are dropped):
[kernel<template arguments>, grid x in threads, grid y, block size, dynamic LDS bytes] -- the numbers as the trace's
`kernels` view reports them (grid_x, grid_y, workgroup_x, lds_size).  tests/test_conv_plan_host.py compares the plans of
csrc/conv_plan.h against these records.
"""
import json
import os
import re
import sqlite3
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS, SETS = ("fwd", "dgrad", "wgrad"), ("all", "teacher640", "student640")


def kernel_name(raw):
    """`conv_igemm_kernel<bf16,128,64,2,2,0,false,false>` from the trace's name, demangled or not (the tracer leaves names
    with a bf16 template argument mangled)."""
    if raw.startswith("_Z"):
        m = re.match(r"_ZN12_GLOBAL__N_1\d+([a-z0-9_]+?)I(.*?)EEv", raw)
        if not m:
            return re.match(r"_ZN12_GLOBAL__N_1\d+([a-z0-9_]+?)E?v?N", raw).group(1)
        args = []
        for tok in re.findall(r"DF16b|Li\d+E|Lb[01]E|f", m.group(2)):
            args.append("bf16" if tok == "DF16b" else "float" if tok == "f" else
                        ("true" if tok[2] == "1" else "false") if tok.startswith("Lb") else tok[2:-1])
        return "%s<%s>" % (m.group(1), ",".join(args))
    name = re.sub(r"\(anonymous namespace\)::|^void ", "", raw)
    name = re.sub(r"\((?:[^()]|\([^()]*\))*\)$", "", name)           # the parameter list
    return name.replace(" ", "").replace("__hip_bfloat16", "bf16")


def main():
    runs = {}
    for k in KINDS:
        for s in SETS:
            c = sqlite3.connect(os.path.join(sys.argv[1], "%s_%s.db" % (k, s)))
            rows = c.execute("select name, grid_x, grid_y, workgroup_x, lds_size from kernels order by start")
            runs["%s_%s" % (k, s)] = [[kernel_name(r[0])] + list(r[1:]) for r in rows if "rocclr" not in r[0]]
    out = os.path.join(HERE, "conv_dispatch_b16.json")
    with open(out, "w") as f:
        f.write('{"record": ["kernel", "grid_x_threads", "grid_y", "block", "lds_bytes"], "batch": 16, "runs": {\n')
        f.write(",\n".join('"%s": [%s]' % (k, ",\n  ".join(json.dumps(r, separators=(",", ":")) for r in v)) for k, v in runs.items()))
        f.write("\n}}\n")
    print(out, {k: len(v) for k, v in runs.items()}, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
