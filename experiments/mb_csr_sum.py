"""csr_sum (sage_csr_sum) on the degree grouping of a graph, beside csr_mean (sage_csr_mean) on the graph itself, and the whole-graph
training step with a trainable embedding (node_degree, 1hot) beside the frozen-table step.

One JSON line per case.  Graph: rmat_graph(20, 16_000_000, seed=0), bench.py's configs[2] graph.
  csr_sum          widths 128 and 256: csr_sum over ops.group_rows(degree, max degree + 1) -- one entry per NODE -- and csr_mean over
                   the graph -- one entry per EDGE -- in ONE process, alternating, device events around each call, median of --reps
                   with min-max.  Both move one table row per entry; the entry counts differ (1.05 M against 30.0 M), so the line
                   gives both times, ns per entry of each, and the ratio of the per-entry costs.
  fullgraph_step   FullGraphTrainer.step at configs[2]'s size (width 256, h1 = h2 = 128, 16 classes, 80 % training rows) with the
                   frozen table, the node_degree embedding (sigmoid) and the 1hot embedding (relu), gcn encoders: --step-reps
                   repetitions of --steps steps each, interleaved, median and range of the per-step time
Run on an MI355X: python experiments/mb_csr_sum.py [--scale 20 --edges 16000000] [--skip-train]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "graphsage-simple_amd")]

from sage355 import ops  # noqa: E402
from sage355.fullgraph import FullGraphTrainer, degree_index, one_hot_index  # noqa: E402
from sage355.graph import rmat_graph  # noqa: E402
from sage355.native import ACT_RELU, ACT_SIGMOID  # noqa: E402


def event_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def stats(ts):
    return {"ms": round(float(np.median(ts)) * 1e3, 3), "ms_min": round(float(np.min(ts)) * 1e3, 3), "ms_max": round(float(np.max(ts)) * 1e3, 3)}


def kernels(g, rp, cl, args):
    n, nnz = g.num_nodes, g.nnz
    index, k = degree_index(rp)
    rp_g, col_g = ops.group_rows(index, k)
    sizes = (rp_g[1:] - rp_g[:-1]).cpu().numpy()
    print(json.dumps({"case": "degree_groups", "nodes": n, "groups": k, "empty_groups": int((sizes == 0).sum()),
                      "long_groups": int((sizes > 512).sum()), "largest": sorted(sizes.tolist())[-3:]}), flush=True)
    for dim in (128, 256):
        x = torch.randn(n, dim, generator=torch.Generator().manual_seed(dim)).cuda()
        out_m = torch.empty(n, dim, device="cuda")
        out_s = torch.empty(k, dim, device="cuda")
        ws_m = torch.empty(ops.csr_mean_workspace_bytes(n, nnz, dim), dtype=torch.uint8, device="cuda")
        ws_s = torch.empty(ops.csr_sum_workspace_bytes(k, n, dim), dtype=torch.uint8, device="cuda")

        def mean():
            ops.csr_mean(rp, cl, x, out=out_m, workspace=ws_m)

        def total():
            ops.csr_sum(rp_g, col_g, x, out=out_s, workspace=ws_s)

        for _ in range(args.warmup):
            mean()
            total()
        torch.cuda.synchronize()
        tm, ts = [], []
        for _ in range(args.reps):                                      # alternating: both see the same state of the box
            tm.append(event_time(mean))
            ts.append(event_time(total))
        m, s = float(np.median(tm)), float(np.median(ts))
        print(json.dumps({"case": "csr_sum", "dim": dim, "reps": args.reps,
                          "csr_mean": dict(stats(tm), entries=nnz, ns_per_entry=round(m / nnz * 1e9, 3)),
                          "csr_sum": dict(stats(ts), entries=n, ns_per_entry=round(s / n * 1e9, 3)),
                          "time_ratio": round(s / m, 4), "per_entry_ratio": round((s / n) / (m / nnz), 3)}), flush=True)
        del x, out_m, out_s, ws_m, ws_s
        torch.cuda.empty_cache()


def training(g, rp, cl, args):
    n = g.num_nodes
    rs = np.random.default_rng(1)
    train = rs.permutation(n)[int(0.2 * n):]
    labels = torch.from_numpy(rs.integers(0, 16, n)).cuda()
    ids = torch.from_numpy(train.astype(np.int32)).cuda()
    tgt = labels[ids.long()]
    table = torch.randn(n, 256, generator=torch.Generator(device="cuda").manual_seed(0), device="cuda")
    common = dict(hidden1=128, hidden2=128, gcn=True, lr=0.05)
    torch.manual_seed(0)
    deg, k = degree_index(rp)
    one, kn = one_hot_index(n, "cuda")
    trainers = {
        "frozen_table": FullGraphTrainer(rp, cl, table, 16, **common),
        "node_degree": FullGraphTrainer(rp, cl, None, 16, embed_index=deg, embed_rows=k, embed_dim=256, act1=ACT_SIGMOID, **common),
        "1hot": FullGraphTrainer(rp, cl, None, 16, embed_index=one, embed_rows=kn, embed_dim=256, act1=ACT_RELU, **common),
    }
    times = {name: [] for name in trainers}
    for tr in trainers.values():
        for _ in range(2):
            tr.step(ids, tgt)
    torch.cuda.synchronize()
    for _ in range(args.step_reps):                                     # interleaved: the three arms see the same state of the box
        for name, tr in trainers.items():
            t0 = time.perf_counter()
            for _ in range(args.steps):
                tr.step(ids, tgt)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.steps)
    base = float(np.median(times["frozen_table"]))
    for name, ts in times.items():
        print(json.dumps(dict({"case": "fullgraph_step", "layer1": name, "graph": f"rmat({args.scale}, {args.edges})", "nodes": n,
                               "train_rows": len(train), "width": 256, "h1": 128, "h2": 128, "steps": args.steps, "reps": args.step_reps,
                               "vs_frozen": round(float(np.median(ts)) / base, 3)}, **stats(ts))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edges", type=int, default=16_000_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--step-reps", type=int, default=20)
    ap.add_argument("--skip-train", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_csr_sum needs an MI355X")
    g = rmat_graph(args.scale, args.edges, seed=0, cache_dir=os.environ.get("SAGE_CACHE", "/tmp/sage_cache"))
    rp, cl = g.to("cuda")
    kernels(g, rp, cl, args)
    if not args.skip_train:
        training(g, rp, cl, args)


if __name__ == "__main__":
    main()
