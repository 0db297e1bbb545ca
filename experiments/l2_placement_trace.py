"""Where does layer 2 run relative to the one-launch layer 1?  Reads a rocprofv3 --kernel-trace CSV of bench.py (gcn encoder, layer 1 as
one phase-sliced launch: stage D is empty), numbers the kernels of every kind in order (= batch index) and reports, over the steady part
of the timed region: the period, every kernel's in-pipeline duration, when L(b) starts relative to G(b)'s end and to G(b+1)'s start,
and the gap between consecutive layer-1 launches.  Layer 1 may alternate over two streams (SAGE_PIPE_G_ALT=1): its launches are numbered by
start time whatever queue they ran in, the queues they used are listed, and the time two of them ran side by side is reported (the gap
between consecutive launches is then negative).  dep_trace.py is the same for the split layer 1 (five kernels per batch).
    python experiments/l2_placement_trace.py <trace dir> [batches of the analysed phase to skip at each end]"""
import collections
import csv
import glob
import sys

import numpy as np

f = sorted(glob.glob(sys.argv[1] + "/**/*_kernel_trace.csv", recursive=True))[-1]
edge = int(sys.argv[2]) if len(sys.argv) > 2 else 40


def kind(n):
    if "sample_kernel" in n:
        return "So" if "true, true>" in n else "Si"
    if "layer1_phase_kernel" in n:
        return "G"
    if "layer_tile16" in n or "layer_fused" in n:
        return "L"
    return None


rows = []
for r in csv.DictReader(open(f)):
    k = kind(r["Kernel_Name"])
    if k:
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), k, r.get("Queue_Id", "?")))
rows.sort()
phases = [[rows[0]]]
last = rows[0][1]
for r in rows[1:]:
    if r[0] - last > 300_000:
        phases.append([])
    phases[-1].append(r)
    last = max(last, r[1])
# warm-up + timed region: the LAST phase of 100 .. 1000 forwards (the preheat phases before it hold thousands)
cands = [ph for ph in phases if 100 * 4 <= len(ph) <= 1000 * 4]
p = cands[-1] if cands else max(phases, key=len)
print("phases (kernels): " + " ".join(str(len(ph)) for ph in phases if len(ph) >= 50))
by = collections.defaultdict(list)
queues = collections.defaultdict(collections.Counter)
for s, e, k, q in p:
    by[k].append((s, e))
    queues[k][q] += 1
# a phase that also holds the preheat (its batches follow one another as closely) or a stray launch of the engine's set-up: the timed
# region is what the phase ENDS with, so the kinds are aligned from the end and at most the last 220 batches are looked at
n = min(220, min(len(v) for v in by.values()))
S = {k: np.array(v[-n:], dtype=np.float64) / 1e3 for k, v in by.items()}     # us
assert all((S["L"][:, 0] > S["G"][:, 0]).tolist()) and all((S["G"][:, 0] > S["Si"][:, 0]).tolist()), "kernel kinds do not line up by batch"
lo, hi = edge, n - edge


def stat(x):
    x = np.asarray(x)
    return "avg %5.1f med %5.1f p10 %5.1f p90 %5.1f" % (x.mean(), np.median(x), np.percentile(x, 10), np.percentile(x, 90))


print(f"analysed phase: {n} batches, statistics over batches {lo} .. {hi - 1}")
print("period %.2f us" % ((S["L"][hi - 1, 1] - S["L"][lo, 1]) / (hi - 1 - lo)))
for k in ("So", "Si", "G", "L"):
    print(f"  {k:2s} duration            {stat(S[k][lo:hi, 1] - S[k][lo:hi, 0])}")
print(f"  L(b) start - G(b) end    {stat(S['L'][lo:hi, 0] - S['G'][lo:hi, 1])}")
print(f"  L(b) start - G(b+1) start{stat(S['L'][lo:hi, 0] - S['G'][lo + 1:hi + 1, 0])}")
print(f"  L(b) end - G(b+1) start  {stat(S['L'][lo:hi, 1] - S['G'][lo + 1:hi + 1, 0])}")
print(f"  G(b+1) start - G(b) end  {stat(S['G'][lo + 1:hi + 1, 0] - S['G'][lo:hi, 1])}")
print(f"  G(b) start - Si(b) end   {stat(S['G'][lo:hi, 0] - S['Si'][lo:hi, 1])}")
print(f"  G(b) and G(b+1) together {stat(np.maximum(0.0, S['G'][lo:hi, 1] - S['G'][lo + 1:hi + 1, 0]))}")
print(f"  G end-to-end period      {stat(np.diff(S['G'][lo:hi + 1, 1]))}")
print("  queues used (whole phase): " + "  ".join(f"{k}: " + ", ".join(f"queue {q} x{c}" for q, c in sorted(queues[k].items())) for k in ("So", "Si", "G", "L")))
t0 = S["G"][lo, 0]
print("  timeline of four batches (us from G(b0) start):")
for b in range(lo, lo + 4):
    print("   b=%d " % b + "  ".join(f"{k} {S[k][b, 0] - t0:7.1f}->{S[k][b, 1] - t0:7.1f}" for k in ("So", "Si", "G", "L")))
