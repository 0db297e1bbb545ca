"""The full-neighbourhood mean reading a trainable embedding through an index (sage_csr_mean_indexed), its grouped backward
(sage_csr_mean_backward_grouped) and the whole-graph node_degree step with FullGraphTrainer(fused_embed=True), each beside what
it replaces.

One JSON line per case.  Graph: rmat_graph(20, 16_000_000, seed=0), bench.py's configs[2] graph; index = degree, K = max degree + 1.
The protocol is experiments/mb_csr_sum.py's: ONE process, the arms alternating, device events around each call, median of --reps
with min-max.  An arm counts as faster only if its whole min-max range lies below the other's ("fused_faster").
  forward          widths 128 and 256: csr_mean(embed, index=degree) against the pair it replaces (index_select into a kept
                   [N, dim] buffer + csr_mean of it) and against csr_mean alone on that materialised table
  backward         widths 128 and 256: csr_mean_backward_grouped against csr_mean_backward + csr_sum over group_rows
  fullgraph_step   FullGraphTrainer.step, node_degree (sigmoid), width 256, h1 = h2 = 128, 16 classes, 80 % training rows, gcn,
                   fused_embed on and off: --step-reps repetitions of --steps steps each, interleaved; and the peak device memory
                   (torch.cuda.max_memory_allocated) of building one trainer and running two steps, above what was allocated before
Run on an MI355X: python experiments/mb_csr_mean_indexed.py [--scale 20 --edges 16000000] [--skip-train]
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "graphsage-simple_amd")]

from sage355 import ops  # noqa: E402
from sage355.fullgraph import FullGraphTrainer, degree_index  # noqa: E402
from sage355.graph import rmat_graph  # noqa: E402
from sage355.native import ACT_SIGMOID  # noqa: E402


def event_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def stats(ts):
    return {"ms": round(float(np.median(ts)) * 1e3, 3), "ms_min": round(float(np.min(ts)) * 1e3, 3), "ms_max": round(float(np.max(ts)) * 1e3, 3)}


def alternate(arms, warmup, reps):
    """{name: fn} -> {name: [seconds]}: every arm once per repetition, in turn."""
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in arms}
    for _ in range(reps):
        for name, fn in arms.items():
            times[name].append(event_time(fn))
    return times


def below(a, b):
    return bool(np.max(a) < np.min(b))


def kernels(g, rp, cl, args):
    n, nnz = g.num_nodes, g.nnz
    index, k = degree_index(rp)
    index64 = index.long()
    groups = ops.group_rows(index, k)
    rp_t, c_t = ops.csr_transpose(rp, cl)
    grouped = ops.csr_transpose_grouped(rp, cl, index, k, self_loop=False)
    sizes = (grouped.rowptr[1:] - grouped.rowptr[:-1]).cpu().numpy()
    print(json.dumps({"case": "grouped_rows", "nodes": n, "edges": nnz, "groups": k, "empty": int((sizes == 0).sum()),
                      "long": int((sizes > 512).sum()), "largest": sorted(sizes.tolist())[-3:]}), flush=True)
    for dim in (128, 256):
        embed = torch.randn(k, dim, generator=torch.Generator().manual_seed(dim)).cuda()
        x = torch.empty(n, dim, device="cuda")
        out = torch.empty(n, dim, device="cuda")
        ws = torch.empty(ops.csr_mean_workspace_bytes(n, nnz, dim), dtype=torch.uint8, device="cuda")

        def select():
            torch.index_select(embed, 0, index64, out=x)

        def mean():
            ops.csr_mean(rp, cl, x, out=out, workspace=ws)

        def pair():
            select()
            mean()

        def indexed():
            ops.csr_mean(rp, cl, embed, out=out, workspace=ws, index=index)

        t = alternate({"indexed": indexed, "index_select+csr_mean": pair, "csr_mean": mean, "index_select": select}, args.warmup, args.reps)
        print(json.dumps({"case": "forward", "dim": dim, "reps": args.reps, **{name: stats(v) for name, v in t.items()},
                          "vs_pair": round(float(np.median(t["indexed"]) / np.median(t["index_select+csr_mean"])), 4),
                          "vs_csr_mean": round(float(np.median(t["indexed"]) / np.median(t["csr_mean"])), 4),
                          "fused_faster_than_pair": below(t["indexed"], t["index_select+csr_mean"]),
                          "fused_faster_than_csr_mean": below(t["indexed"], t["csr_mean"])}), flush=True)
        del embed, out, ws

        g_out = x.normal_(generator=torch.Generator(device="cuda").manual_seed(dim))
        g_x = torch.empty(n, dim, device="cuda")
        g_e = torch.empty(k, dim, device="cuda")
        ws_b = torch.empty(ops.csr_mean_backward_workspace_bytes(n, n, nnz, dim), dtype=torch.uint8, device="cuda")
        ws_s = torch.empty(ops.csr_sum_workspace_bytes(k, n, dim), dtype=torch.uint8, device="cuda")
        ws_g = torch.empty(ops.csr_mean_backward_grouped_workspace_bytes(n, k, grouped.col.numel(), dim), dtype=torch.uint8, device="cuda")

        def two():
            ops.csr_mean_backward(rp, cl, rp_t, c_t, g_out, out=g_x, workspace=ws_b)
            ops.csr_sum(groups[0], groups[1], g_x, out=g_e, workspace=ws_s)

        def one():
            ops.csr_mean_backward_grouped(rp, cl, grouped, g_out, out=g_e, workspace=ws_g)

        t = alternate({"grouped": one, "csr_mean_backward+csr_sum": two}, args.warmup, args.reps)
        print(json.dumps({"case": "backward", "dim": dim, "reps": args.reps, **{name: stats(v) for name, v in t.items()},
                          "vs_pair": round(float(np.median(t["grouped"]) / np.median(t["csr_mean_backward+csr_sum"])), 4),
                          "fused_faster": below(t["grouped"], t["csr_mean_backward+csr_sum"])}), flush=True)
        del x, g_out, g_x, g_e, ws_b, ws_s, ws_g
        torch.cuda.empty_cache()


def training(g, rp, cl, args):
    n = g.num_nodes
    rs = np.random.default_rng(1)
    train = rs.permutation(n)[int(0.2 * n):]
    labels = torch.from_numpy(rs.integers(0, 16, n)).cuda()
    ids = torch.from_numpy(train.astype(np.int32)).cuda()
    tgt = labels[ids.long()]
    deg, k = degree_index(rp)

    def make(fused):
        torch.manual_seed(0)
        return FullGraphTrainer(rp, cl, None, 16, hidden1=128, hidden2=128, gcn=True, lr=0.05, embed_index=deg, embed_rows=k, embed_dim=256,
                                act1=ACT_SIGMOID, fused_embed=fused)

    peak = {}
    for fused in (False, True):                                         # one trainer alive at a time: what ONE arm needs
        gc.collect()
        torch.cuda.empty_cache()
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        tr = make(fused)
        for _ in range(2):
            tr.step(ids, tgt)
        torch.cuda.synchronize()
        peak[fused] = torch.cuda.max_memory_allocated() - before
        del tr
    trainers = {"unfused": make(False), "fused": make(True)}
    times = {name: [] for name in trainers}
    for tr in trainers.values():
        for _ in range(2):
            tr.step(ids, tgt)
    torch.cuda.synchronize()
    for _ in range(args.step_reps):                                     # interleaved: both arms see the same state of the box
        for name, tr in trainers.items():
            t0 = time.perf_counter()
            for _ in range(args.steps):
                tr.step(ids, tgt)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.steps)
    print(json.dumps({"case": "fullgraph_step", "layer1": "node_degree", "graph": f"rmat({args.scale}, {args.edges})", "nodes": n,
                      "train_rows": len(train), "width": 256, "h1": 128, "h2": 128, "steps": args.steps, "reps": args.step_reps,
                      "unfused": dict(stats(times["unfused"]), peak_mib=round(peak[False] / 2**20, 1)),
                      "fused": dict(stats(times["fused"]), peak_mib=round(peak[True] / 2**20, 1)),
                      "ratio": round(float(np.median(times["fused"]) / np.median(times["unfused"])), 4),
                      "fused_faster": below(times["fused"], times["unfused"])}), flush=True)


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
        raise SystemExit("mb_csr_mean_indexed needs an MI355X")
    g = rmat_graph(args.scale, args.edges, seed=0, cache_dir=os.environ.get("SAGE_CACHE", "/tmp/sage_cache"))
    rp, cl = g.to("cuda")
    kernels(g, rp, cl, args)
    if not args.skip_train:
        training(g, rp, cl, args)


if __name__ == "__main__":
    main()
