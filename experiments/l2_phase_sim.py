"""Ideal-LRU simulation of the bytes the layer-1 gather reads past the eight L2s at BASELINE config 3, for the column-sliced gather
(XCD x caches slice x of every destination row) and for the phase-sliced layer 1 (csrc/sage_layer1_phase.hip: XCD x owns an eighth of the
destination rows and walks the 8 slices in 8 phases, L2 taken as cold per phase).  32 Ki lines of 128 B per XCD, two batches.
Result (CPU, a few seconds after the graph build): sliced gather 153-155 MB past the L2s (55 % hits; measured on the part: 171 MB,
52 %), phase form 212-215 MB (38 % hits).  Net of the 48 MB round trip of the means the phase form is at +11 MB: bytes break even.
"""
import os, sys, time
import numpy as np
_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(_HERE), "graphsage-simple_amd"))
sys.path.insert(0, os.path.join(_HERE, "r03"))
from sage355.graph import rmat_graph, relabel_by_degree
from l2_caps_sim import sample_rows, lru_misses
t=time.time()
g = relabel_by_degree(rmat_graph(20, 16_000_000, seed=0, cache_dir=os.environ.get("SAGE_CACHE_DIR"), accel=None))[0]
print("graph", time.time()-t, flush=True)
rng = np.random.default_rng(1)
cand = np.nonzero(g.degrees() > 0)[0]
cap = 32768
for trial in range(2):
    seeds = rng.choice(cand, size=4096, replace=False)
    s1 = np.unique(np.concatenate(sample_rows(g, seeds, 25, rng)))
    rng.shuffle(s1)
    rows = sample_rows(g, s1, 15, rng)
    e1 = sum(len(x) for x in rows)
    allsrc = np.concatenate(rows)
    uniq = len(np.unique(allsrc))
    print(f"trial {trial}: S1={len(s1)} E1={e1} uniq={uniq} compulsory {uniq*1024/1e6:.1f} MB per-edge {e1*1024/1e6:.1f} MB")
    m = lru_misses(allsrc, cap)
    print(f"  today (one XCD sees all rows' slice, cold LRU 32Ki): {m*1024/1e6:.1f} MB hits {1-m/e1:.1%}")
    idx = np.arange(len(rows))
    for nparts, label in ((8, "8 XCD x 8 phases of 128B"), (4, "4 XCD-pairs x 4 phases of 256B (pair shares rows; each XCD half)")):
        tot = 0
        for x in range(nparts):
            part = [rows[i] for i in idx[(idx // 4) % nparts == x]]
            st = np.concatenate(part)
            mm = lru_misses(st, cap)
            tot += mm
            if x == 0: print(f"    part0: edges {len(st)} uniq {len(np.unique(st))} lru-miss {mm}")
        print(f"  {label}: reads {tot*1024/1e6:.1f} MB (hits {1-tot/e1:.1%}); minus means round trip 48 MB -> net vs today {tot*1024/1e6 - m*1024/1e6 - 48:+.1f} MB")
