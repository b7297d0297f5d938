"""k_expr_eval throughput probe: a*b + c over N Float64 rows (24 B read +
8 B write per row) through a terminal Projection with device-resident input,
next to a device-to-device copy that moves the same bytes (N * 16 B read +
N * 16 B written).

Run it under a kernel trace of its own and read the two kernels' times from
the stats:

    rocprofv3 --kernel-trace --stats -d DIR -o expr -- \\
        python tools/bench_expr.py --rows 67108864

The script itself prints wall-clock figures only as a sanity check; the
kernel times come from the trace.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))

import torch  # noqa: E402

import blaze_amd  # noqa: E402
from blaze_amd import plan  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64 << 20)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    n = args.rows
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(7)
    a, b, c = (torch.rand(n, dtype=torch.float64, device=dev, generator=g)
               for _ in range(3))
    fields = [plan.field(nm, plan.DT_FLOAT64, False) for nm in "abc"]
    expr = plan.binary_expr(
        plan.binary_expr(plan.column("a", 0), plan.column("b", 1),
                         "Multiply"),
        plan.column("c", 2), "Plus")
    task = plan.task_definition(plan.projection(
        plan.ffi_reader(fields, "input0"), [expr], ["r"]))
    for rep in range(args.reps):
        db = blaze_amd.DeviceBatch(
            [{"ptr": t.data_ptr(), "len": n} for t in (a, b, c)])
        t0 = time.perf_counter()
        t = blaze_amd.Task(task, device_batches=[db.as_input()])
        outs = t.run()
        dt = time.perf_counter() - t0
        t.finalize()
        if rep == 0:  # spot check against torch, separately rounded
            want = (a[:4096] * b[:4096]).add(c[:4096]).cpu().numpy()
            assert (outs[0][0]["values"][:4096] == want).all()
        print(f"[bench_expr] task rep {rep}: {dt * 1e3:.1f} ms wall "
              f"(includes the {n * 8 >> 20} MiB result download)")
    # the same byte volume as one d2d copy: n*16 B read, n*16 B written
    src = torch.empty(n * 2, dtype=torch.float64, device=dev).fill_(1.0)
    dst = torch.empty_like(src)
    for rep in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dst.copy_(src)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(f"[bench_expr] d2d copy rep {rep}: {dt * 1e3:.3f} ms wall, "
              f"{n * 32 / dt / 1e9:.0f} GB/s read+write")


if __name__ == "__main__":
    main()
