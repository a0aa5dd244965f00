#!/usr/bin/env python3
"""The idle time between back-to-back cycle windows, from a rocprofv3 kernel trace of bench.py:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python bench.py --gpus 1 --steps 50 --warmup 50
    python scripts/window_gap.py DIR/NAME_kernel_trace.csv [timed windows, default 50]

A window of the headline V-cycle starts with the finest level's `-1` node: the dispatch of the streaming kernel with the
fused restriction on the largest grid.  For the last K windows of the trace (the timed ones) this prints the gap from the end of the last
kernel of a window to the start of the first kernel of the next one, the window period, and the k_finish_batch
dispatches per window."""
import csv
import statistics
import sys


def main(path, K=50):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"],
                         int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) * int(r["Grid_Size_Z"])))
    rows.sort()
    # the `-1` nodes: streaming dispatches with the fused restriction (4th template argument); the finest one has the largest grid
    down = [i for i, r in enumerate(rows) if "k_jacobi_stream<" in r[2] and r[2].split("<", 1)[1].split(",")[3].strip() == "true"]
    top = max(rows[i][3] for i in down)
    starts = [i for i in down if rows[i][3] == top]
    starts = starts[-K:]
    gaps = [(rows[i][0] - rows[i - 1][1]) * 1e-3 for i in starts[1:]]
    period = [(rows[b][0] - rows[a][0]) * 1e-3 for a, b in zip(starts, starts[1:])]
    busy = [sum(rows[i][1] - rows[i][0] for i in range(a, b)) * 1e-3 for a, b in zip(starts, starts[1:])]
    finish = [sum(1 for i in range(a, b) if "k_finish_batch" in rows[i][2]) for a, b in zip(starts, starts[1:])]
    launches = [b - a for a, b in zip(starts, starts[1:])]
    q = lambda v: f"median {statistics.median(v):.2f}  min {min(v):.2f}  max {max(v):.2f}"
    print(f"{path}: {len(gaps)} boundaries between the last {len(starts)} windows")
    print(f"  gap, last kernel of a window -> first kernel of the next (us): {q(gaps)}")
    print(f"  window period, start to start (us):                            {q(period)}")
    print(f"  time inside kernels per window (us):                           {q(busy)}")
    print(f"  dispatches per window: {statistics.median(launches)}   k_finish_batch per window: {statistics.median(finish)} (min {min(finish)}, max {max(finish)})")


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 50)
