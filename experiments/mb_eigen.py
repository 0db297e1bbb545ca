"""One Chebyshev step (sage_csr_cheb_step) beside the composed form the library offered before it, and one whole ops.eigen_top call.

One JSON line per case.  Graph: rmat_graph(20, 16_000_000, seed=0), bench.py's configs[2] graph (symmetric).
  cheb_step   native: one sage_csr_cheb_step call on a planned graph, out = a S + b y + g x written over x's block (the form
              ops.eigen_top's filter runs).  composed: ops.csr_sum into a block of its own (it plans on every call), then the three
              in-place torch passes mul_(a), add_(y, alpha=b), add_(x, alpha=g).  ONE process, alternating, after --warmup rounds,
              device events around each, median of --reps with min-max, at every --dims width.  `compulsory_bytes` is what a step
              must move once (col 4 E, rowptr 8 N, y and x read and out written 12 N dim; the gathered rows of y are counted ONCE,
              as if every re-read hit a cache), `share_of_hbm_peak` those bytes over the native time over 8 TB/s: a byte rate of
              the whole step named as such, not a kernel's counter.  `max_abs_diff_over_scale` compares the two results (the
              composed form rounds a S before it adds); `plain_product_bits_equal`: a = 1, b = g = 0 against ops.csr_sum, bit for bit.
  gram        is torch.mm(X^T, X) at [N, 120] the same bits three times over, in fp32 and in fp64?  (ops.eigen_top's "same
              arguments, same bits" rests on it.)
  eigen_top   one whole ops.eigen_top(k = --k, tol = --tol, max_iter = --max-iter) call: outer iterations, A.X products, host clock
              around the synchronised call, the device time inside csr_cheb_step (events around every call) and so the share of
              everything else (the dense torch algebra, the host's m x m factorizations and their syncs), peak memory allocated,
              the residual history relative to theta_1.  A run that does not converge within --max-iter is reported as such.
Run on an MI355X: python experiments/mb_eigen.py [--scale 20 --edges 16000000]
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


def step_case(g, rp, cl, dim, args, a=0.031, b=-0.43, c=-0.97):
    n, e = g.num_nodes, g.nnz
    plan = ops.csr_cheb_plan(rp, cl, dim)
    gen = torch.Generator(device="cuda").manual_seed(dim)
    y = torch.randn(n, dim, generator=gen, device="cuda")
    x0 = torch.randn(n, dim, generator=gen, device="cuda")
    x, s = x0.clone(), torch.empty(n, dim, device="cuda")
    ws = torch.empty(ops.csr_sum_workspace_bytes(n, e, dim), dtype=torch.uint8, device="cuda")

    def native_step():
        ops.csr_cheb_step(plan, y, x=x, a=a, b=b, g=c, out=x)

    def composed():
        ops.csr_sum(rp, cl, y, out=s, workspace=ws)
        s.mul_(a).add_(y, alpha=b).add_(x0, alpha=c)

    for _ in range(args.warmup):
        x.copy_(x0)
        native_step()
        composed()
    torch.cuda.synchronize()
    tn, tc = [], []
    for _ in range(args.reps):                                          # alternating: both see the same state of the box
        x.copy_(x0)
        tn.append(event_time(native_step))
        tc.append(event_time(composed))
    diff = float((x - s).abs().max() / s.abs().max())
    plain = torch.equal(ops.csr_cheb_step(plan, y, out=x).view(torch.int32), ops.csr_sum(rp, cl, y, out=s, workspace=ws).view(torch.int32))
    need = 4 * e + 8 * n + 12 * n * dim
    t = float(np.median(tn))
    print(json.dumps({"case": "cheb_step", "dim": dim, "nodes": n, "entries": e, "reps": args.reps, "native": stats(tn), "composed": stats(tc),
                      "composed_over_native": round(float(np.median(tc)) / t, 3), "compulsory_bytes": need,
                      "bytes_per_second": round(need / t / 1e12, 3), "share_of_hbm_peak": round(need / t / HBM_PEAK, 4),
                      "gathered_row_bytes": 4 * e * dim, "max_abs_diff_over_scale": diff, "plain_product_bits_equal": bool(plain)}), flush=True)


def gram_case(g):
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(g.num_nodes, 120, generator=gen, device="cuda")
    out = {}
    for name, t in (("fp32", x), ("fp64", x[:, :100].double())):
        first = torch.mm(t.t(), t)
        out[name] = all(torch.equal(first, torch.mm(t.t(), t)) for _ in range(3))
    print(json.dumps({"case": "gram", "nodes": g.num_nodes, "same_bits_three_times": out}), flush=True)


def whole_case(g, rp, cl, args):
    spans = []
    inner = ops.csr_cheb_step

    def timed(*a, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = inner(*a, **kw)
        e1.record()
        spans.append((e0, e1))
        return r

    ops.csr_cheb_step = timed
    hist, result, error = [], None, None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    try:
        result = ops.eigen_top(rp, cl, args.k, tol=args.tol, max_iter=args.max_iter, degree=args.degree, history=hist)
    except native.SageError as err:
        error = str(err)
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    ops.csr_cheb_step = inner
    steps = sum(a.elapsed_time(b) for a, b in spans) * 1e-3
    row = {"case": "eigen_top", "nodes": g.num_nodes, "entries": g.nnz, "k": args.k, "tol": args.tol, "degree": args.degree,
           "max_iter": args.max_iter, "converged": result is not None, "iterations": len(hist), "products": len(spans),
           "seconds": round(total, 3), "seconds_in_steps": round(steps, 3), "share_outside_steps": round(1 - steps / total, 3),
           "ms_per_product": round(steps / max(len(spans), 1) * 1e3, 3),
           "peak_allocated_gb": round((torch.cuda.max_memory_allocated() - before) / 1e9, 3), "error": error}
    if result is not None:
        values, vectors, _ = result
        row.update(theta_1=float(values[0]), theta_k=float(values[-1]), residual_over_theta_1=[round(h / float(values[0]), 8) for h in hist],
                   vectors_bits_sum=int(vectors.view(torch.int32).to(torch.int64).sum()))
    else:
        row.update(residual_history=[float(h) for h in hist])
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edges", type=int, default=16_000_000)
    ap.add_argument("--dims", type=int, nargs="*", default=[100, 120, 128, 256])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--degree", type=int, default=10)
    ap.add_argument("--max-iter", type=int, default=40)
    ap.add_argument("--skip-whole", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_eigen needs an MI355X")
    g = rmat_graph(args.scale, args.edges, seed=0, cache_dir=os.environ.get("SAGE_CACHE", "/tmp/sage_cache"))
    rp, cl = g.to("cuda")
    for dim in args.dims:
        step_case(g, rp, cl, dim, args)
    gram_case(g)
    if not args.skip_whole:
        whole_case(g, rp, cl, args)


if __name__ == "__main__":
    main()
