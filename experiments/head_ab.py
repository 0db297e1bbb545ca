"""EngineTrainer step time with head="torch" against head="native" (DESIGN.md section 8): the eager and the captured step on the stand-in
Cora (1433 -> 50 -> 128, fanout 10/10, 256 seeds, 7 classes) and at config-3 size (R-MAT 2^20 / 16 M edges, D0 = 256, H = 128/128, fanout
15/25, 4096 seeds, 16 classes: the setup of train_big.py).  Both heads in one process, alternating, --reps repetitions each: medians and
the spread.  The two heads share every other kernel, so the "torch" rows are what the step cost before the native head existed.

  python experiments/head_ab.py                 # both setups, JSON on the last line
  python experiments/head_ab.py --head-only     # only sage_xent_head in a loop at the two shapes (for a kernel trace of its two kernels)
"""
import argparse, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "graphsage-simple_amd")]
import numpy as np, torch
from sage355 import ops
from sage355.datasets import standin_citation
from sage355.graph import CSRGraph, rmat_graph
from sage355.train import EngineTrainer

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--head-only", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda", 0)


def head_alone(n, dim, c, iters=300):
    """Device time of one sage_xent_head call (row kernel + reduce), from events around `iters` back-to-back calls."""
    gen = torch.Generator(device=dev).manual_seed(0)
    emb = torch.randn(n, dim, generator=gen, device=dev)
    w = torch.randn(c, dim, generator=gen, device=dev) / dim ** 0.5
    labels = torch.randint(0, c, (n,), generator=gen, device=dev)
    ws = torch.empty(ops.xent_head_workspace_bytes(n, dim, c), dtype=torch.uint8, device=dev)
    out = ops.xent_head(emb, w, labels, workspace=ws)
    for _ in range(20):
        ops.xent_head(emb, w, labels, workspace=ws, out=out)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(5):
        a.record()
        for _ in range(iters):
            ops.xent_head(emb, w, labels, workspace=ws, out=out)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / iters)
    return {"shape": [n, dim, c], "us_per_call_median": float(np.median(ts)), "us_min": min(ts), "us_max": max(ts)}


def summary(ts):
    return {"median_us": round(float(np.median(ts)) * 1e6, 1), "min_us": round(min(ts) * 1e6, 1), "max_us": round(max(ts) * 1e6, 1), "reps": len(ts)}


def ab(name, make, ring, keys, labels_by_node):
    heads = ("torch", "native")
    trs = {}
    for h in heads:
        torch.manual_seed(0)
        trs[h] = make(h)
    nring = ring.shape[0]
    lab = [labels_by_node[ring[i].long()] for i in range(nring)]
    eager = {h: [] for h in heads}
    for h in heads:
        for i in range(10):
            trs[h].step(ring[i % nring], lab[i % nring], keys[i % nring])
    for rep in range(args.reps):
        for h in (heads if rep % 2 == 0 else heads[::-1]):
            tr = trs[h]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                tr.step(ring[i % nring], lab[i % nring], keys[i % nring])
            torch.cuda.synchronize()
            eager[h].append((time.perf_counter() - t0) / args.steps)
    captured = {h: [] for h in heads}
    for h in heads:
        trs[h].capture_step(ring, keys, labels_by_node)
        for _ in range(10):
            trs[h].replay_step()
    for rep in range(args.reps):
        for h in (heads if rep % 2 == 0 else heads[::-1]):
            tr = trs[h]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                tr.replay_step()
            torch.cuda.synchronize()
            captured[h].append((time.perf_counter() - t0) / args.steps)
    last = {h: float(trs[h].replay_step()) for h in heads}
    res = {"setup": name, "last_loss": last, "eager": {h: summary(eager[h]) for h in heads}, "captured": {h: summary(captured[h]) for h in heads}}
    print(json.dumps(res), flush=True)
    return res


results = {"head_alone": [head_alone(256, 128, 7), head_alone(4096, 128, 16)]}
print(json.dumps(results["head_alone"]), flush=True)
if not args.head_only:
    z = np.load(os.path.join(REPO, "tests", "golden", "cora_topology.npz"))
    g = CSRGraph(z["rowptr"], z["col"], len(z["rowptr"]) - 1)
    feats, labels = standin_citation(g, num_classes=7, feat_dim=1433, seed=0)
    table = torch.from_numpy(feats).to(dev)
    rowptr, col = g.to(dev)
    rs = np.random.default_rng(0)
    ring = torch.from_numpy(np.stack([rs.choice(g.num_nodes, 256, replace=False) for _ in range(16)]).astype(np.int32)).to(dev)
    results["cora_256"] = ab("stand-in Cora, 256 seeds",
                             lambda h: EngineTrainer(rowptr, col, table, 7, hidden1=50, hidden2=128, num_sample1=10, num_sample2=10, gcn=True, lr=0.7,
                                                     max_batch=256, head=h),
                             ring, list(range(16)), torch.from_numpy(labels.reshape(-1)).to(dev))
    g = rmat_graph(20, 16_000_000, seed=0, cache_dir=os.environ.get("SAGE_CACHE", "/tmp/sage_cache"))
    gen = torch.Generator(device=dev).manual_seed(0)
    table = torch.randn(g.num_nodes, 256, generator=gen, device=dev)
    labels_by_node = (table @ torch.randn(256, 16, generator=gen, device=dev)).argmax(1)
    rowptr, col = g.to(dev)
    cand = np.nonzero(g.degrees() > 0)[0]
    rs = np.random.default_rng(1)
    ring = torch.from_numpy(np.stack([rs.choice(cand, 4096, replace=False) for _ in range(32)]).astype(np.int32)).to(dev)
    results["config3_4096"] = ab("config 3, 4096 seeds",
                                 lambda h: EngineTrainer(rowptr, col, table, 16, hidden1=128, hidden2=128, num_sample1=15, num_sample2=25, gcn=True,
                                                         lr=0.05, max_batch=4096, relabel="degree", head=h),
                                 ring, [500 + i for i in range(32)], labels_by_node)
print(json.dumps(results))
