#!/usr/bin/env python3
"""The GroupNorm statistics pass at the level-0 launch of the full-size forward (n_slabs = 50, rows = 9216, C = 320, split
input): ew_groupnorm_stats_f16 + ew_groupnorm_finalize, ITERS times after a warm-up.  Prints the event-timed mean per pass;
per-kernel times come from a kernel trace of the same command:
    rocprofv3 --kernel-trace --output-format csv -d out -- python tools/bench_groupnorm_stats.py
    python tools/csv_kernel_stats.py out/*/*kernel_trace.csv
EW_LIB_PATH selects another build of the library (A/B against the parent commit's in one session)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from evoworld_amd import _lib, ops  # noqa: E402

DEV = "cuda"
N_SLABS, ROWS, C, GROUPS = 50, 9216, 320, 32
ITERS = int(os.environ.get("EW_GN_ITERS", "50"))

lib = _lib.load()
x = ops.Res.from_float(torch.randn(N_SLABS * ROWS, C, device=DEV, generator=torch.Generator(DEV).manual_seed(0)) * 1.5 + 0.3)
ws = torch.empty(lib.ew_groupnorm_workspace_floats(N_SLABS, ROWS, C, GROUPS), dtype=torch.float32, device=DEV)


def one_pass():
    ops._call("ew_groupnorm_stats_f16", ops._ptr(x.hi), ops._ptr(x.lo), ops._ptr(ws), N_SLABS, ROWS, C, 0, C, GROUPS)
    ops._call("ew_groupnorm_finalize", ops._ptr(ws), N_SLABS, ROWS, C, GROUPS)


for _ in range(5):
    one_pass()
torch.cuda.synchronize()
s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
s.record()
for _ in range(ITERS):
    one_pass()
e.record()
torch.cuda.synchronize()
us = s.elapsed_time(e) * 1e3 / ITERS
stats = ws[-N_SLABS * GROUPS * 2:].double().reshape(N_SLABS, GROUPS, 2)
print(f"groupnorm statistics pass {N_SLABS} x {ROWS} x {C} (hi + lo8): {us:.1f} us per stats + finalize over {ITERS} passes, "
      f"{N_SLABS * ROWS * C * 3 / us / 1e6:.2f} TB/s; mean of means {float(stats[..., 0].mean()):.6f}, of variances {float(stats[..., 1].mean()):.6f} "
      f"(library: {os.environ.get('EW_LIB_PATH') or 'in-tree'})")
