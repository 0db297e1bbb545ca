"""Full-neighbourhood mean (sage_csr_mean) and whole-graph inference (sage355.inference) at configs[2]'s size.

One JSON line per case.  Graph: rmat_graph(20, 16_000_000, seed=0), bench.py's configs[2] graph (30.0 M CSR entries over
1,048,576 nodes, max degree 62,333, median 1); table 256 wide, h1 = h2 = 128.  Times: device events around the call, after
warm-up, median of --reps.  Rates are ALGORITHMIC bytes over that time: every CSR entry's table row + col + rowptr + out.
  csr_mean      all nodes on the R-MAT graph, and on a graph of the same N and nnz with near-uniform degrees
  skew          time per byte on R-MAT / time per byte on the uniform graph (the split rule's target: <= 1.3)
  embed         embed_all_nodes, gcn and concat encoders: time and embeddings / s
  parity        the max-degree row and 64 random rows of h1 and out against an fp64 recomputation on the CPU
Run on an MI355X: python experiments/mb_csr_mean.py [--scale 20 --edges 16000000]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "graphsage-simple_amd")]

from sage355 import ops  # noqa: E402
from sage355.graph import rmat_graph  # noqa: E402
from sage355.inference import _nonempty_flag, embed_all_nodes  # noqa: E402


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def mean_bytes(n, nnz, dim):
    return nnz * (4 * dim + 4) + (n + 1) * 8 + n * 4 * dim


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edges", type=int, default=16_000_000)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_csr_mean needs an MI355X")
    g = rmat_graph(args.scale, args.edges, seed=0)
    n, nnz, d0, h = g.num_nodes, g.nnz, args.dim, args.hidden
    deg = g.degrees()
    gen = torch.Generator().manual_seed(0)
    table = torch.randn(n, d0, generator=gen).cuda()
    rp, cl = g.to("cuda")
    flag = _nonempty_flag(rp)
    out = torch.empty(n, d0, device="cuda")
    ws = torch.empty(ops.csr_mean_workspace_bytes(n, nnz, d0), dtype=torch.uint8, device="cuda")

    def run_mean(rp_, cl_):
        return lambda: ops.csr_mean(rp_, cl_, table, any_nonempty=flag, out=out, workspace=ws)

    t, tmin, tmax = timed(run_mean(rp, cl), args.warmup, args.reps)
    by = mean_bytes(n, nnz, d0)
    print(json.dumps({"case": "csr_mean", "graph": f"rmat({args.scale}, {args.edges})", "nodes": n, "nnz": nnz, "max_degree": int(deg.max()),
                      "dim": d0, "ms": round(t * 1e3, 3), "ms_min": round(tmin * 1e3, 3), "ms_max": round(tmax * 1e3, 3),
                      "alg_GB": round(by / 1e9, 2), "TBps": round(by / t / 1e12, 2)}), flush=True)
    # same N and nnz, near-uniform degrees
    rng = np.random.default_rng(1)
    udeg = np.full(n, nnz // n, dtype=np.int64)
    udeg[rng.choice(n, nnz - int(udeg.sum()), replace=False)] += 1
    urp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(udeg, out=urp[1:])
    ucl = rng.integers(0, n, nnz, dtype=np.int64).astype(np.int32)
    urp_d, ucl_d = torch.from_numpy(urp).cuda(), torch.from_numpy(ucl).cuda()
    del ucl
    tu, _, _ = timed(run_mean(urp_d, ucl_d), args.warmup, args.reps)
    print(json.dumps({"case": "csr_mean", "graph": "uniform", "nodes": n, "nnz": nnz, "max_degree": int(udeg.max()), "dim": d0,
                      "ms": round(tu * 1e3, 3), "TBps": round(by / tu / 1e12, 2)}), flush=True)
    print(json.dumps({"case": "skew", "ratio": round(t / tu, 3), "target": 1.3}), flush=True)
    del urp_d, ucl_d, out, ws
    torch.cuda.empty_cache()

    for concat in (False, True):
        m = 2 if concat else 1
        w1 = (torch.randn(h, m * d0, generator=gen) / (m * d0) ** 0.5).cuda()
        w2 = (torch.randn(h, m * h, generator=gen) / (m * h) ** 0.5).cuda()
        res = torch.empty(n, h, device="cuda")
        hidden = torch.empty(n, h, device="cuda")

        def embed():
            return embed_all_nodes(rp, cl, table, w1, w2, concat=concat, out=res)

        te, _, _ = timed(embed, args.warmup, max(5, args.reps // 4))
        print(json.dumps({"case": "embed_all_nodes", "encoder": "concat" if concat else "gcn", "nodes": n, "d0": d0, "h1": h, "h2": h,
                          "ms": round(te * 1e3, 3), "emb_per_s": round(n / te, 1)}), flush=True)
        # spot parity: h1 from the same call layer by layer, rows against fp64
        from sage355.inference import layer_all_nodes
        layer_all_nodes(rp, cl, table, w1, concat, False, ops.ACT_RELU, out=hidden)
        torch.cuda.synchronize()
        rows = np.concatenate([[int(np.argmax(deg))], rng.choice(np.nonzero(deg > 0)[0], 64, replace=False)])
        t64, h64 = table.cpu().double(), hidden.cpu().double()
        W1, W2 = w1.cpu().double(), w2.cpu().double()
        err1 = err2 = 0.0
        for v in rows:
            nb = torch.from_numpy(g.neighbors(int(v)).astype(np.int64))
            a1 = t64[nb].mean(0)
            x1 = torch.cat([t64[v], a1]) if concat else a1
            r1 = torch.relu(W1 @ x1)
            a2 = h64[nb].mean(0)
            x2 = torch.cat([h64[v], a2]) if concat else a2
            r2 = torch.relu(W2 @ x2)
            err1 = max(err1, ((hidden[v].cpu().double() - r1).abs().max() / r1.abs().max().clamp_min(1e-30)).item())
            err2 = max(err2, ((res[v].cpu().double() - r2).abs().max() / r2.abs().max().clamp_min(1e-30)).item())
        print(json.dumps({"case": "parity", "encoder": "concat" if concat else "gcn", "rows": len(rows),
                          "max_degree_row": int(rows[0]), "h1_err_rowmax": err1, "out_err_rowmax": err2, "bar": 1e-5}), flush=True)
        del res, hidden
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
