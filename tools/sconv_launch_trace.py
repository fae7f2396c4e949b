#!/usr/bin/env python
"""Which kernel instantiation, grid, workgroup and LDS size does every launch of the forward get, under every setting of
egonn_debug_set_naive_conv?  Two steps:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/sconv_launch_trace.py
    python tools/sconv_launch_trace.py --list DIR OUT.txt [NAME-FILTER]
The first runs, per setting, one eager forward of the smoke batch of tests/test_gpu_launch_tags.py and one egonn_sparse_conv per
map kind on a two-scan plan; a setting starts with one erfinv launch (nothing else uses it).  The second writes the ordered
launches of the library's kernels (those whose name holds NAME-FILTER), `[count x] name<template arguments> | grid (workgroups) |
workgroup | static LDS bytes` per run of equal launches under a `# setting` header: two trees launch the same things exactly when
their lists are equal line for line (profiles/sconv_choice_trace.txt is the list with the filter `sconv`;
tests/test_sconv_choice_host.py takes its literals from there)."""
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (name, precision, exact fp32, code): the three product settings, then every accepted code of include/egonn_hip.h
SETTINGS = [("fp32", "fp32", False, 0), ("fp32_exact", "fp32", True, 0), ("bf16", "bf16", False, 0)] + \
           [(f"code{c}", "fp32", False, c) for c in (1, 2, 4, 8, 16, 32, 128, 1142, 1182, 1183, 1542, 1942, 9142)]
# one stand-alone convolution per map kind: (kind, output level, cin, cout)
CONVS = [(0, 1, 32, 32), (1, 3, 64, 64), (2, 3, 128, 128)]


def run():
    import numpy as np
    import torch
    import __graft_entry__ as entry
    entry.build()
    import egonn_amd as E
    from egonn_amd import _lib
    from egonn_amd.synth import lidar_scan, seeded_state_dict
    model = E.model_factory(E.ModelParams(model="egonn", coordinates="cartesian", quantization_step=0.1))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(7, shapes).items()})
    model = model.to("cuda:0").eval()
    scans = [lidar_scan(2 + i, n_points=6000) for i in range(2)]
    off = [0, len(scans[0]), len(scans[0]) + len(scans[1])]
    pts = torch.from_numpy(np.concatenate(scans)).cuda()
    ex = E.DescriptorExtractor(model, n_k=128)
    ctx = model.context(0)
    one = _lib.Context(coord_bits=12)
    one.voxelize(pts, off, 0, [0.1])
    torch.manual_seed(0)
    operands = []
    for kind, lvl, ci, co in CONVS:
        n_in = one.level_count(lvl if kind == 0 else (lvl - 1 if kind == 1 else lvl + 1))
        operands.append((torch.randn(n_in, ci, device="cuda"), torch.randn(27 if kind == 0 else 8, ci, co, device="cuda") * 0.05))
    mark = torch.full((64,), 0.5, device="cuda")
    for name, precision, exact, code in SETTINGS:
        torch.cuda.synchronize()
        mark.clone().erfinv_()
        model.precision = precision
        ctx.set_exact_fp32(exact)
        ctx.set_naive_conv(code)
        one.set_naive_conv(code)
        try:
            ex.extract_packed(pts, off)
            for (kind, lvl, ci, co), (x, w) in zip(CONVS, operands):
                try:
                    one.sparse_conv(kind, lvl, x, w)
                except _lib.EgonnError as e:           # a refused combination launches nothing: part of the record
                    print(f"[{name}] conv kind {kind} L{lvl} {ci}->{co}: {e}", flush=True)
        except _lib.EgonnError as e:
            print(f"[{name}] forward: {e}", flush=True)
        ctx.set_naive_conv(0)
        one.set_naive_conv(0)
    ctx.set_exact_fp32(False)
    torch.cuda.synchronize()
    print("done", flush=True)


def listing(src, out, only="egonn::"):
    rows = []
    for path in glob.glob(os.path.join(src, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            rows += list(csv.DictReader(f))
    assert rows, f"no *kernel_trace.csv under {src}"
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [s[0] for s in SETTINGS]
    lines, seg, count = [], -1, 0
    for r in rows:
        name = r["Kernel_Name"]
        if "erfinv" in name:
            seg += 1
            lines.append([1, f"# {names[seg]}"])
        elif seg >= 0 and "egonn::" in name and only in name:
            wg = [int(r[f"Workgroup_Size_{a}"]) for a in "XYZ"]
            grid = [int(r[f"Grid_Size_{a}"]) // w for a, w in zip("XYZ", wg)]
            name = name.removeprefix("void ").replace("egonn::", "")
            if name.endswith(")"):                       # drop the argument list: the template arguments stay
                depth, j = 0, len(name) - 1
                while j >= 0:
                    depth += {")": 1, "(": -1}.get(name[j], 0)
                    if depth == 0:
                        break
                    j -= 1
                name = name[:j]
            line = f"{name} | {grid[0]} x {grid[1]} x {grid[2]} | {wg[0]} | {r['LDS_Block_Size']}"
            count += 1
            if lines[-1][1] == line:                     # consecutive equal launches: one line, counted
                lines[-1][0] += 1
            else:
                lines.append([1, line])
    assert seg == len(names) - 1, f"{seg + 1} settings in the trace, {len(names)} expected"
    with open(out, "w") as f:
        f.write("".join((f"{n} x " if n > 1 else "") + line + "\n" for n, line in lines))
    print(f"{count} launches of {len(names)} settings -> {out}")


if __name__ == "__main__":
    if len(sys.argv) in (4, 5) and sys.argv[1] == "--list":
        listing(*sys.argv[2:])
    else:
        run()
