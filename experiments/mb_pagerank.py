"""One PageRank step (sage_pagerank_step) beside the composed form the library offered before it, and the whole ops.pagerank call.

One JSON line per case.  Graph: rmat_graph(20, 16_000_000, seed=0), bench.py's configs[2] graph (symmetric: its CSR is its pull CSR).
  pagerank_step    native: one sage_pagerank_step call on ping-pong buffers (chunk pass, step kernel, fixed-order reduce).
                   composed: y = x * inv_out, ops.csr_sum at dim = 1, the dangling mass and err as torch sums, the update as torch
                   element-wise ops.  ONE process, alternating, after --warmup rounds, device events around each, median of --reps
                   with min-max.  `compulsory_bytes` is what a step must move once (col 4 E, rowptr 8 N, x / inv_out read and x_next /
                   y_next written 16 N; the gathered y is counted ONCE, 4 N, as if every re-read hit a cache), `share_of_hbm_peak` is
                   those bytes over the native time over 8 TB/s: a byte rate of the whole step named as such, not a kernel's counter.
                   `max_rel_diff` compares the two x_next (they add in different orders); `x_next_bits_sum` is the sum of the native
                   x_next's bit patterns: builds with other -DSAGE_PAGERANK_GROUP / -DSAGE_PAGERANK_ROWS (SAGE355_LIB names the
                   library to load) must print the same number.
  pagerank         the whole ops.pagerank call (allocation, init, every step with its 4-byte err read), host clock around a
                   synchronised call, median of --runs.
Run on an MI355X: python experiments/mb_pagerank.py [--scale 20 --edges 16000000]
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

from sage355 import native, ops  # noqa: E402
from sage355.graph import rmat_graph  # noqa: E402

HBM_PEAK = 8.0e12


def event_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def stats(ts):
    return {"ms": round(float(np.median(ts)) * 1e3, 4), "ms_min": round(float(np.min(ts)) * 1e3, 4), "ms_max": round(float(np.max(ts)) * 1e3, 4)}


def step_case(g, rp, cl, args, alpha=0.85):
    n, e = g.num_nodes, g.nnz
    L, P = native.lib(), native.ptr
    xs, ys = torch.empty(2, n, device="cuda"), torch.empty(2, n, device="cuda")
    inv_out, state = torch.empty(n, device="cuda"), torch.empty(2, device="cuda")
    ws = torch.empty(ops.pagerank_workspace_bytes(n, e), dtype=torch.uint8, device="cuda")
    native.check(L.sage_pagerank_init(P(rp), n, e, None, P(xs[0]), P(ys[0]), P(inv_out), P(state), P(ws), ws.numel(), native.stream_handle()))
    start_state = state.clone()

    def step():
        native.check(L.sage_pagerank_step(P(rp), P(cl), n, e, P(inv_out), alpha, P(xs[0]), P(ys[0]), P(xs[1]), P(ys[1]), P(state), P(ws), ws.numel(),
                                          native.stream_handle()))

    ws_sum = torch.empty(ops.csr_sum_workspace_bytes(n, e, 1), dtype=torch.uint8, device="cuda")
    s = torch.empty(n, 1, device="cuda")
    dangling = inv_out == 0
    out = {}

    def composed():
        x = xs[0]
        y = x * inv_out
        ops.csr_sum(rp, cl, y.view(n, 1), out=s, workspace=ws_sum)
        mass = torch.where(dangling, x, 0.0).sum()
        x_next = alpha * (s.view(n) + mass / n) + (1.0 - alpha) / n
        out["y_next"] = x_next * inv_out
        out["err"] = (x_next - x).abs().sum()
        out["x_next"] = x_next

    for _ in range(args.warmup):
        state.copy_(start_state)
        step()
        composed()
    torch.cuda.synchronize()
    tn, tc = [], []
    for _ in range(args.reps):                                          # alternating: both see the same state of the box
        state.copy_(start_state)                                        # every native step starts from x_0's mass
        tn.append(event_time(step))
        tc.append(event_time(composed))
    rel = float(((xs[1] - out["x_next"]).abs() / out["x_next"]).max())
    lens = np.diff(g.rowptr)
    need = 4 * e + 8 * n + 16 * n + 4 * n
    t = float(np.median(tn))
    print(json.dumps({"case": "pagerank_step", "nodes": n, "entries": e, "rows_over_chunk": int((lens > native.CSR_MEAN_CHUNK).sum()),
                      "dangling": int((lens == 0).sum()), "reps": args.reps, "native": stats(tn), "composed": stats(tc),
                      "composed_over_native": round(float(np.median(tc)) / t, 3), "compulsory_bytes": need,
                      "bytes_per_second": round(need / t / 1e12, 3), "share_of_hbm_peak": round(need / t / HBM_PEAK, 4),
                      "err_native": float(state[0]), "err_composed": float(out["err"]), "max_rel_diff": rel,
                      "x_next_bits_sum": int(xs[1].view(torch.int32).to(torch.int64).sum())}), flush=True)


def whole_case(g, rp, cl, args):
    ops.pagerank(rp, cl)
    torch.cuda.synchronize()
    ts, it = [], 0
    for _ in range(args.runs):
        t0 = time.perf_counter()
        x, it = ops.pagerank(rp, cl)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    print(json.dumps(dict({"case": "pagerank", "nodes": g.num_nodes, "entries": g.nnz, "iterations": it, "runs": args.runs,
                           "ms_per_iteration": round(float(np.median(ts)) * 1e3 / it, 4), "sum_x": float(x.double().sum())}, **stats(ts))),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edges", type=int, default=16_000_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_pagerank needs an MI355X")
    g = rmat_graph(args.scale, args.edges, seed=0, cache_dir=os.environ.get("SAGE_CACHE", "/tmp/sage_cache"))
    rp, cl = g.to("cuda")
    step_case(g, rp, cl, args)
    whole_case(g, rp, cl, args)


if __name__ == "__main__":
    main()
