"""The touched-rows embedding gradient and sparse SGD update against the dense path of the same build, at
configs[2]'s graph (R-MAT 2^20 / 16 M edges, B = 4096, fanout 15/25, width 256, H = 128/128).  Both sides of each comparison in one
process, alternating, --reps repetitions: median (min - max).

  (a) sage_embed_grad + embed.add_(g, alpha=-lr) against ONE sage_embed_grad_rows call that applies the update (and the same call
      also returning the compact gradient), on the same (g_agg1, nbr1, cnt1) taken from one forward, for the identity index
      (R = 2^20) and the degree index (R = max degree + 1).  The dense side writes into a gradient allocated once, which the
      trainer's step does not do: (b) has that cost.
  (b) EngineTrainer.step, dense against sparse_embed=True, for both indices, with each step's peak allocation above what is resident
  (c) --big: (a) for the identity batch with every id multiplied by 8 in a table of R = 2^23 rows (configs[3]'s node count): the same
      terms, eight times the rows

  python experiments/mb_embed_sparse.py                  # JSON on the last line
  python experiments/mb_embed_sparse.py --kernel-only --only identity    # only (a), one index: for a kernel trace of the launches
"""
import argparse, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "graphsage-simple_amd")]
import numpy as np, torch
from sage355 import ops
from sage355.engine import TwoHopEngine
from sage355.fullgraph import degree_index, one_hot_index
from sage355.graph import rmat_graph
from sage355.train import EngineTrainer

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--kernel-only", action="store_true")
ap.add_argument("--big", action="store_true")
ap.add_argument("--only", choices=["identity", "degree"], default=None, help="one index only (a kernel trace per index)")
args = ap.parse_args()
dev = torch.device("cuda", 0)
B, K1, K2, D0, H, LR = 4096, 15, 25, 256, 128, 0.05


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


def kernel_ab(name, rowptr, col, index, rows, seeds, spread=1):
    gen = torch.Generator(device=dev).manual_seed(0)
    small = torch.randn(rows, D0, generator=gen, device=dev)
    w1 = torch.randn(H, D0, generator=gen, device=dev) / D0 ** 0.5
    w2 = torch.randn(H, H, generator=gen, device=dev) / H ** 0.5
    eng = TwoHopEngine(rowptr, col, small, w1, w2, K1, K2, max_batch=B, embed_index=index)
    eng.forward(seeds, seed=7)
    it = eng.intermediates()
    ws = eng._ws_views()
    n1 = eng.layout.max_s1
    nbr1, cnt1, s1 = ws("nbr1"), ws("cnt1"), ws("s1_nodes")
    if spread > 1:                                                     # the same terms in a table `spread` times as long
        nbr1, rows = (nbr1 * spread).contiguous(), rows * spread
    nlive = torch.tensor([it["n_s1"]], dtype=torch.int32, device=dev)
    g = torch.randn(n1, D0, generator=gen, device=dev)
    order = ops.row_order(s1, n_dev=nlive)
    start = torch.randn(rows, D0, generator=gen, device=dev)
    tables = {k: start.clone() for k in ("dense", "update", "rows+update")}
    del start, small
    g_dense = torch.empty(rows, D0, device=dev)
    cap = min(n1 * K1, rows)
    out = (torch.empty(cap, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev), torch.empty(cap, D0, device=dev))
    ws_dense = torch.empty(ops.embed_grad_workspace_bytes(n1, K1, rows, D0), dtype=torch.uint8, device=dev)
    ws_rows = torch.empty(ops.embed_grad_rows_workspace_bytes(n1, K1, rows, D0), dtype=torch.uint8, device=dev)

    def dense():
        ops.embed_grad(g, nbr1, cnt1, rows, n_dev=nlive, row_order=order, out=g_dense, workspace=ws_dense)
        tables["dense"].add_(g_dense, alpha=-LR)

    def update():
        ops.embed_grad_rows(g, nbr1, cnt1, rows, n_dev=nlive, row_order=order, embed=tables["update"], lr=LR, want_grad=False,
                            out=(None, out[1], None), workspace=ws_rows)

    def rows_update():
        ops.embed_grad_rows(g, nbr1, cnt1, rows, n_dev=nlive, row_order=order, embed=tables["rows+update"], lr=LR, out=out, workspace=ws_rows)

    sides = (("dense", dense), ("update", update), ("rows+update", rows_update))
    for _, fn in sides:
        fn()
    torch.cuda.synchronize()
    touched = int(out[1])
    scale = g_dense.abs().max().item()
    diff = (tables["dense"] - tables["update"]).abs().max().item() / scale     # 0 where add_(g, alpha=) is a fused multiply-add, as the kernel's update is
    same_grad = bool(torch.equal(g_dense[out[0][:touched].long()], out[2][:touched]))
    ts = {k: [] for k, _ in sides}
    for rep in range(args.reps):
        for k, fn in (sides if rep % 2 == 0 else sides[::-1]):
            ts[k].append(timed(fn, args.iters))
    terms = int(torch.minimum(cnt1[:it["n_s1"]], torch.tensor(K1, device=dev)).sum())
    res = {"index": name, "embed_rows": rows, "layer1_rows": it["n_s1"], "terms": terms, "touched_rows": touched, "max_rel_diff_of_tables": diff,
           "compact_gradient_bit_equal": same_grad,
           "workspace_MiB": {"embed_grad": round(ws_dense.numel() / 2 ** 20, 1), "embed_grad_rows": round(ws_rows.numel() / 2 ** 20, 1)},
           **{k: summary(v) for k, v in ts.items()}}
    print(json.dumps(res), flush=True)
    return res


def step_ab(name, rowptr, col, index, rows, act1, ring, labels_by_node):
    kw = dict(hidden1=H, hidden2=H, num_sample1=K1, num_sample2=K2, gcn=True, lr=LR, max_batch=B, embed_index=index, embed_rows=rows,
              embed_dim=D0, act1=act1)
    trs = {}
    for k, sparse in (("dense", False), ("sparse", True)):
        torch.manual_seed(0)
        trs[k] = EngineTrainer(rowptr, col, None, 16, sparse_embed=sparse, **kw)
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
    res = {"index": name, "embed_rows": rows, "step": {k: summary(v, 1e6) for k, v in ts.items()}, "step_peak_MiB_above_resident": peak,
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
want = lambda name: args.only in (None, name)
results = {"kernel": ([kernel_ab("identity", rowptr, col, one_index, one_rows, ring[0])] if want("identity") else []) +
                     ([kernel_ab("degree", rowptr, col, deg_index, deg_rows, ring[0])] if want("degree") else [])}
if args.big:
    results["kernel"].append(kernel_ab("identity x 8", rowptr, col, one_index, one_rows, ring[0], spread=8))
if not args.kernel_only:
    results["step"] = ([step_ab("identity", rowptr, col, one_index, one_rows, ops.ACT_RELU, ring, labels_by_node)] if want("identity") else []) + \
                      ([step_ab("degree", rowptr, col, deg_index, deg_rows, ops.ACT_SIGMOID, ring, labels_by_node)] if want("degree") else [])
print(json.dumps(results))
