"""What separates two consecutive full-chip kernels: the queue they share, or the event the first carries?  (mb_boundary.hip)
    hipcc -O3 -fPIC -shared --offload-arch=gfx950 experiments/mb_boundary.hip -o experiments/mb_boundary.so
    python experiments/mb_boundary.py [kernel_us=40] [chain=24] [repeats=5] [json out]
Prints, per way and setting, start(i+1) - end(i) over the chain (median, p10, p90 over all repeats, the first two links of every chain
left out: the host is still ahead of nothing there) and the kernel's own duration."""
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
lib = ctypes.CDLL(os.path.join(HERE, "mb_boundary.so"))
D = ctypes.POINTER(ctypes.c_double)
lib.run_boundary.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, D, D, D]
kernel_us = float(sys.argv[1]) if len(sys.argv) > 1 else 40.0
n = int(sys.argv[2]) if len(sys.argv) > 2 else 24
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
WAYS = ["one stream, plain", "one stream, stop event", "two streams, plain", "two streams, stop event", "one stream, timed start+stop"]


def stat(x):
    return {"median": round(float(np.median(x)), 2), "p10": round(float(np.percentile(x, 10)), 2), "p90": round(float(np.percentile(x, 90)), 2)}


table = []
for beside in (0, 1):
    for way, name in enumerate(WAYS):
        gaps, durs, egaps = [], [], []
        for _ in range(repeats):
            g, d, e = (ctypes.c_double * (n - 1))(), (ctypes.c_double * n)(), (ctypes.c_double * (n - 1))()
            rc = lib.run_boundary(way, beside, n, kernel_us, g, d, e)
            if rc != 0:
                sys.exit(f"run_boundary(way={way}, beside={beside}) failed")
            gaps += list(g)[2:]
            durs += list(d)[2:]
            egaps += list(e)[2:] if way == 4 else []
        row = {"way": name, "beside": bool(beside), "gap_us": stat(gaps), "duration_us": stat(durs)}
        if egaps:
            row["gap_us_by_events"] = stat(egaps)
        table.append(row)
        print("%-30s %-7s gap %6.2f (%6.2f .. %6.2f)  kernel %6.2f (%6.2f .. %6.2f)%s" % (
            name, "beside" if beside else "idle", row["gap_us"]["median"], row["gap_us"]["p10"], row["gap_us"]["p90"],
            row["duration_us"]["median"], row["duration_us"]["p10"], row["duration_us"]["p90"],
            "  by events %6.2f" % row["gap_us_by_events"]["median"] if egaps else ""), flush=True)
if len(sys.argv) > 4:
    json.dump({"kernel_us": kernel_us, "chain": n, "repeats": repeats, "rows": table}, open(sys.argv[4], "w"), indent=1)
