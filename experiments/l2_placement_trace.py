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
    if "layer1_phase_kernel" in n or "layer1_pair_kernel" in n:
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
# (no such phase: the preheat runs into the timed region, or the bench repeats it; then the LAST phase of at least 100 forwards, not
# the longest one, which may be a preheat of its own that ends in a drained pipe)
big = [ph for ph in phases if len(ph) >= 100 * 4]
p = cands[-1] if cands else big[-1] if big else max(phases, key=len)
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

# ---- round 11: which constraint binds each kernel start?  (dep_trace.py's idea for the four-kernel pipeline.)  A kernel can start once
# every one of its constraints is met: the previous kernel of its queue has ended, its producer has ended, and for So the workspace
# has been released by L(b - depth).  The LAST of them to be met is the binding one; the distance from it to the start is what the
# hand-off (or the queue's boundary) cost.  The queue of a kernel is the one the trace names, so the table follows whatever cut of the
# four streams the library made: Si in stream S's queue behind So, or in a layer-1 queue in front of G.
depth = int(sys.argv[3]) if len(sys.argv) > 3 else 4
ev = sorted((s, e, k, q, i) for k in ("So", "Si", "G", "L") for i, ((s, e), q) in enumerate(zip(by[k][-n:], [r[3] for r in p if r[2] == k][-n:])))
prev_in_queue, last_of_queue = {}, {}
for s, e, k, q, i in ev:
    prev_in_queue[(k, i)] = last_of_queue.get(q)
    last_of_queue[q] = (k, i, e / 1e3)
Q = {(k, i): q for s, e, k, q, i in ev}
producer = {"Si": "So", "G": "Si", "L": "G"}
binding = {k: collections.Counter() for k in ("So", "Si", "G", "L")}
slack = {k: collections.defaultdict(list) for k in ("So", "Si", "G", "L")}
bound_by = {}
for k in ("So", "Si", "G", "L"):
    for b in range(lo, hi):
        start = S[k][b, 0]
        cons = {}
        pq = prev_in_queue[(k, b)]
        if pq:
            cons["queue:%s(b%+d)" % (pq[0], pq[1] - b)] = pq[2]
        if k in producer:
            cons["producer:%s(b)" % producer[k]] = S[producer[k]][b, 1]
        if k == "So" and b - depth >= 0:
            cons["release:L(b-%d)" % depth] = S["L"][b - depth, 1]
        name, t = max(cons.items(), key=lambda kv: kv[1])
        binding[k][name] += 1
        bound_by[(k, b)] = name
        slack[k][name].append(start - t)
print(f"last constraint met before each kernel start (batches {lo} .. {hi - 1}; depth {depth}): count, then start - constraint in us")
for k in ("So", "Si", "G", "L"):
    for name, c in binding[k].most_common():
        print(f"  {k:2s} <- {name:18s} x{c:4d} ({100.0 * c / (hi - lo):5.1f} %)  {stat(slack[k][name])}")
# a layer-1 start held by stream S's own chain: G(b) waited for Si(b), which waited for So(b), which waited for its queue (not the release)
chain = sum(1 for b in range(lo, hi) if bound_by[("G", b)].startswith("producer:Si") and bound_by[("Si", b)].startswith(("queue:So", "producer:So"))
            and bound_by[("So", b)].startswith("queue:"))
print(f"  layer-1 starts whose last constraints lead back through Si(b) and So(b) to So(b)'s queue predecessor: {chain} of {hi - lo} ({100.0 * chain / (hi - lo):.1f} %)")
print(f"  So(b+1) start - Si(b) end  {stat(S['So'][lo + 1:hi + 1, 0] - S['Si'][lo:hi, 1])}")
print(f"  Si(b) start - So(b) end    {stat(S['Si'][lo:hi, 0] - S['So'][lo:hi, 1])}")
print(f"  G(b) start - Si(b) end     {stat(S['G'][lo:hi, 0] - S['Si'][lo:hi, 1])}")
print(f"  So(b) start - L(b-{depth}) end   {stat(S['So'][lo:hi, 0] - S['L'][lo - depth:hi - depth, 1])}")
print(f"  L(b+1) start - L(b) end    {stat(S['L'][lo + 1:hi + 1, 0] - S['L'][lo:hi, 1])}")
# each queue's busy time, and busy time plus the boundary in front of every kernel that followed its queue predecessor's end within
# 30 us (a longer distance is a wait for data, not a boundary), as a share of the period
period = (S["L"][hi - 1, 1] - S["L"][lo, 1]) / (hi - 1 - lo)
busy, bound, kinds = collections.Counter(), collections.Counter(), collections.defaultdict(collections.Counter)
for s, e, k, q, i in ev:
    if lo <= i < hi:
        busy[q] += (e - s) / 1e3
        kinds[q][k] += 1
        pq = prev_in_queue[(k, i)]
        if pq and 0.0 < s / 1e3 - pq[2] < 30.0:
            bound[q] += s / 1e3 - pq[2]
print("  per queue, per batch of the pipe: busy us, busy + boundary us, share of the period")
for q in sorted(busy):
    what = " ".join(f"{k} x{c}" for k, c in sorted(kinds[q].items()))
    print(f"   queue {q}: busy {busy[q] / (hi - lo):5.1f}  busy + boundary {(busy[q] + bound[q]) / (hi - lo):5.1f}  = {100.0 * (busy[q] + bound[q]) / (hi - lo) / period:5.1f} % of {period:.1f}   ({what})")
