"""The embedding's gradient on the sampled engine path, at configs[2]'s graph (R-MAT 2^20 / 16 M edges, B = 4096,
fanout 15/25, width 256, H = 128/128).  Both sides of each comparison in one process, alternating, --reps repetitions: median (min - max).

  (a) sage_embed_grad against sage_gather_mean_backward_ws (one lane group walks a destination row's whole run) on the same
      (g_agg1, nbr1, cnt1, R) taken from one forward, for the degree index (R = max degree + 1) and the identity index (R = N)
  (b) an EngineTrainer step with a degree embedding of width 256 against the frozen-table step, with each step's peak memory

  python experiments/mb_embed_grad.py                  # JSON on the last line
  python experiments/mb_embed_grad.py --kernel-only    # only (a): for a kernel trace of the two entry points' launches
"""
import argparse, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "graphsage-simple_amd")]
import numpy as np, torch
from sage355 import native, ops
from sage355.engine import TwoHopEngine
from sage355.fullgraph import degree_index, one_hot_index
from sage355.graph import rmat_graph
from sage355.train import EngineTrainer

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--kernel-only", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda", 0)
B, K1, K2, D0, H = 4096, 15, 25, 256, 128


def summary(ts, unit=1.0):
    return {"median_us": round(float(np.median(ts)) * unit, 1), "min_us": round(min(ts) * unit, 1), "max_us": round(max(ts) * unit, 1), "reps": len(ts)}


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def kernel_ab(name, rowptr, col, index, rows, seeds):
    gen = torch.Generator(device=dev).manual_seed(0)
    embed = torch.randn(rows, D0, generator=gen, device=dev)
    w1 = torch.randn(H, D0, generator=gen, device=dev) / D0 ** 0.5
    w2 = torch.randn(H, H, generator=gen, device=dev) / H ** 0.5
    eng = TwoHopEngine(rowptr, col, embed, w1, w2, K1, K2, max_batch=B, embed_index=index)
    eng.forward(seeds, seed=7)
    it = eng.intermediates()
    ws = eng._ws_views()
    n1 = eng.layout.max_s1
    nbr1, cnt1, s1 = ws("nbr1"), ws("cnt1"), ws("s1_nodes")
    nlive = torch.tensor([it["n_s1"]], dtype=torch.int32, device=dev)
    g = torch.randn(n1, D0, generator=gen, device=dev)
    order = ops.row_order(s1, n_dev=nlive)
    out_new = torch.empty(rows, D0, device=dev)
    out_old = torch.empty(rows, D0, device=dev)
    L, P, st = native.lib(), native.ptr, native.stream_handle()
    ws_new = torch.empty(ops.embed_grad_workspace_bytes(n1, K1, rows, D0), dtype=torch.uint8, device=dev)
    ws_old = torch.empty(L.sage_gather_mean_backward_workspace_bytes(n1, K1, rows), dtype=torch.uint8, device=dev)

    def new():
        ops.embed_grad(g, nbr1, cnt1, rows, n_dev=nlive, row_order=order, out=out_new, workspace=ws_new)

    def old():
        native.check(L.sage_gather_mean_backward_ws(P(g), D0, D0, P(nbr1), P(cnt1), K1, n1, P(nlive), None, None, P(out_old), rows, None, D0,
                                                    P(ws_old), ws_old.numel(), st), "gather_mean_backward_ws")

    sides = (("embed_grad", new), ("gather_mean_backward_ws", old))
    for _, fn in sides:
        fn()
    torch.cuda.synchronize()
    scale = out_old.abs().max().item()
    diff = (out_new - out_old).abs().max().item() / scale       # the two orders differ; the sums agree to rounding
    ts = {k: [] for k, _ in sides}
    for rep in range(args.reps):
        for k, fn in (sides if rep % 2 == 0 else sides[::-1]):
            ts[k].append(timed(fn, args.iters))
    terms = int(torch.minimum(cnt1[:it["n_s1"]], torch.tensor(K1, device=dev)).sum())
    res = {"index": name, "embed_rows": rows, "layer1_rows": it["n_s1"], "terms": terms, "max_rel_diff": diff,
           "workspace_MiB": {"embed_grad": round(ws_new.numel() / 2 ** 20, 1), "gather_mean_backward_ws": round(ws_old.numel() / 2 ** 20, 1)},
           **{k: summary(v) for k, v in ts.items()}}
    print(json.dumps(res), flush=True)
    return res


def step_ab(rowptr, col, n, index, rows, ring, labels_by_node):
    gen = torch.Generator(device=dev).manual_seed(0)
    table = torch.randn(n, D0, generator=gen, device=dev)
    kw = dict(hidden1=H, hidden2=H, num_sample1=K1, num_sample2=K2, gcn=True, lr=0.05, max_batch=B)
    torch.manual_seed(0)
    trs = {"frozen": EngineTrainer(rowptr, col, table, 16, **kw)}
    torch.manual_seed(0)
    trs["degree_embedding"] = EngineTrainer(rowptr, col, None, 16, embed_index=index, embed_rows=rows, embed_dim=D0, act1=ops.ACT_SIGMOID, **kw)
    nring = ring.shape[0]
    lab = [labels_by_node[ring[i].long()] for i in range(nring)]
    names = tuple(trs)
    ts, peak = {k: [] for k in names}, {}
    for k in names:
        for i in range(10):
            trs[k].step(ring[i % nring], lab[i % nring], 500 + i)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        trs[k].step(ring[0], lab[0], 500)
        torch.cuda.synchronize()
        peak[k] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)       # MiB a step allocates above what is resident
    for rep in range(args.reps):
        for k in (names if rep % 2 == 0 else names[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                trs[k].step(ring[i % nring], lab[i % nring], 500 + i)
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) / args.steps)
    res = {"step": {k: summary(v, 1e6) for k, v in ts.items()}, "step_peak_MiB_above_resident": peak,
           "last_loss": {k: float(trs[k].step(ring[0], lab[0], 500)) for k in names}}
    print(json.dumps(res), flush=True)
    return res


g = rmat_graph(20, 16_000_000, seed=0, cache_dir=os.environ.get("SAGE_CACHE", "/tmp/sage_cache"))
rowptr, col = g.to(dev)
cand = np.nonzero(g.degrees() > 0)[0]
rs = np.random.default_rng(1)
ring = torch.from_numpy(np.stack([rs.choice(cand, B, replace=False) for _ in range(16)]).astype(np.int32)).to(dev)
labels_by_node = torch.from_numpy(rs.integers(0, 16, g.num_nodes)).to(dev)
deg_index, deg_rows = degree_index(rowptr)
one_index, one_rows = one_hot_index(g.num_nodes, dev)
results = {"kernel": [kernel_ab("degree", rowptr, col, deg_index, deg_rows, ring[0]),
                      kernel_ab("identity", rowptr, col, one_index, one_rows, ring[0])]}
if not args.kernel_only:
    results.update(step_ab(rowptr, col, g.num_nodes, deg_index, deg_rows, ring, labels_by_node))
print(json.dumps(results))
